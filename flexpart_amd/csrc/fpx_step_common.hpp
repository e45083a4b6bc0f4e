// What the engine and the three kernels of the particle step (timemanager.f90:531-712: fpx_step_prep.hpp, fpx_step_loop.hpp)
// share: the block size, the keys of the work-list sort and the layout of its counters, the tuning macros (register budgets
// of the step kernels, schedule of the Langevin launches), how a kernel reads its View in place, the set-up of a particle's
// random-number source, the epilogue of a particle's step (timemanager.f90:630-708) and the per-slot hand-over record
// between k_prep, k_pbl_loop and k_pbl_finish.  No kernel lives here.
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#include <cstddef>

namespace fpx {
FPX_TU_OPEN

constexpr int kBlock = 256;
// The big kernels read the fields of their first argument, the View, THROUGH the kernel-argument segment instead of from the
// by-value parameter.  A by-value aggregate is a private copy that the optimiser splits into one scalar per field, all loaded at the
// kernel's entry: in k_prep that is 40 scalar loads whose results do not fit the scalar file and travel as lanes of a vector
// register (800-1300 v_readlane per kernel; polar k_prep 0.78 instead of 0.71 ms) -- and as soon as ONE access has an address
// the optimiser cannot resolve (a per-lane subscript, a select between two fields' addresses) the whole copy lives in scratch
// (576-816 B per lane in three instance families before this).  Read in place, every field is a scalar load from constant memory
// next to its use, re-loaded rather than spilled, and no copy exists that could end up in scratch.  The View must be the kernel's
// FIRST parameter (offset 0 of the segment).
#ifndef FPX_VIEW_BY_VALUE
#define FPX_VIEW_FROM_KERNARG(V, V_arg) const View<R> &V = *(const View<R> *)(const void *)__builtin_amdgcn_kernarg_segment_ptr(); (void)V_arg
#else
#define FPX_VIEW_FROM_KERNARG(V, V_arg) const View<R> &V = V_arg
#endif
#ifndef FPX_PREP_WAVES
#define FPX_PREP_WAVES 3   // register budget (waves per SIMD) of k_prep (<= 168 VGPRs)
#endif
#ifndef FPX_INIT_PREP_3WAVES
#define FPX_INIT_PREP_3WAVES 1    // the INIT instance of k_prep at the three-wave budget too: its initialize() body runs only in waves that hold a new particle
#endif
#ifndef FPX_PREP_TWO_WAVES   // which instances of k_prep keep the two-wave register budget: none since the arguments are read in place (the nest
// instances fit 168 VGPRs without a spill, the ones with dry deposition spill 6-12 registers; round 3: every INIT / POLAR / NEST / DRYDEP instance at two waves)
#define FPX_PREP_TWO_WAVES(INIT, POLAR, NEST, DRYDEP) ((INIT && !FPX_INIT_PREP_3WAVES) || (POLAR && !FPX_POLAR_PREP_3WAVES))
#endif
#ifndef FPX_POLAR_PREP_3WAVES
#define FPX_POLAR_PREP_3WAVES 1   // the polar instance of k_prep at the three-wave register budget (the polar move is out of line: polar_move)
#endif
#ifndef FPX_FINISH_WAVES
#define FPX_FINISH_WAVES 2 // register budget of k_pbl_finish
#endif
#ifndef FPX_LOOP_WAVES_F32
#define FPX_LOOP_WAVES_F32 4   // the f32 instances fit 128 VGPRs: four waves per SIMD (measured: 168 -> 184 ms at 1e8 when they slipped to three)
#endif
#ifndef FPX_LOOP_WAVES
#define FPX_LOOP_WAVES 3   // waves per SIMD the Langevin kernel is register-budgeted for (<= 168 VGPRs)
#endif
#ifndef FPX_COST_BUCKETS
#define FPX_COST_BUCKETS -1  // the work list orders each class by the expected number of passes, longest first (k_prep): -1 = for clouds below 5e7 particles
#endif
#ifndef FPX_SLICE_SCHEDULE
#define FPX_SLICE_SCHEDULE 0   // pass budgets of the successive launches of the Langevin kernel, 0 = none; one entry = ONE launch (measured best)
#endif
#ifndef FPX_DRAIN_LANES
#define FPX_DRAIN_LANES 32   // a wave of a non-final launch whose list is used up hands its particles on when fewer lanes than this hold one
#endif
constexpr int kMaxNz = 512;
constexpr unsigned char kKeyDone = 32, kKeyNotDue = 33;   // keys of the work-list sort (6 bits); 0..31: PBL particles, class-major (k_prep)

// ---------------------------------------------------------------------------
// the hot kernels: one pass of the particle loop timemanager.f90:531-712
//
//   k_prep : every due particle -- initialize() if newly released, grid/cell/PBL test;
//            particles above the PBL finish here (one interpol_wind step + Petterssen:
//            gather/stream bound); PBL particles are appended to a work list.
//   k_pbl  : persistent waves over the work list.  Each lane owns one PBL particle and runs
//            passes of the Langevin loop; a lane whose particle has finished its lsynctime
//            immediately refills from the list, so lanes never idle on the data-dependent
//            trip count (15-150 passes per particle).
// ---------------------------------------------------------------------------
template <typename R, typename RNG>
__device__ __forceinline__ void make_rng(const View<R> &V, unsigned int pid, unsigned int step, RNG &G) {
  G.tab = V.rannumb; G.maxrand = V.maxrand; G.mode = V.rng_mode;
  G.pid = pid + V.pid_base; G.step = step;
  G.k0 = (unsigned int)V.seed; G.k1 = (unsigned int)(V.seed >> 32);
  G.cblk = 0xffffffffu;
}

template <typename R>
__device__ __forceinline__ int advance_start_index(const View<R> &V, const SeqRng &S, const Rng<R> &G, unsigned int pid) {
  if (V.rng_mode == 0) return S.nrand_adv[pid];      // advance.f90:153, serial stream replayed by the host
  if (V.rng_mode == 1) return G.start_index(0);
  return 1;
}

// epilogue timemanager.f90:630-708 + write-back of the particle
// TURB: also write up, vp, cbt -- changed only by initialize() and by the Langevin loop; a particle that
// was above the mixing layer for the whole step keeps them (advance.f90:629-708 does not touch them)
// What the epilogue reads of the particle itself (release point, masses): fetched by the caller together with its last
// gather (EpiPre::load inside a `late` hook), so that the epilogue starts with them instead of with two more dependent
// memory round trips at the tail of a latency-bound kernel.
// (the release point and the first species' mass: three registers; the kernels have none to spare for more)
template <typename R>
struct EpiPre {
  int npoint;
  R xm0;
  template <bool DRYDEP>
  __device__ __forceinline__ void load(const View<R> &V, const GridP<R> &Gp, const Parts<R> &P, long long s) {
    const bool massfract = V.mdomainfill == 0 && V.mquasilag == 0;
    npoint = ((massfract && V.numpoint > 1) || (DRYDEP && Gp.on)) ? P.npoint[s] : 1;
    xm0 = P.xmass1[s];
  }
};

// the dry deposition of one particle's step, handed back to a caller that scatters it where its wave is convergent again
// (k_pbl_finish: the neighbourhood sums of wave_kernel_add need every lane of the wave)
template <typename R>
struct DryDep {
  float dep[kMaxSpec];   // drydeposit(ks), timemanager.f90:650-656,690-693 (0: nothing)
  R x, y;                // the particle's position the kernel is centred on (xtra1, ytra1 after the step)
  int nage, kp, nclass;
};

template <typename R, bool DRYDEP, bool TURB = true>
__device__ __forceinline__ void epilogue_store(const View<R> &V, const GridP<R> &Gp, Parts<R> &P, long long s, int itime, int itramem,
                                               int nstop, const PState<R> &ps, const R *prob, Stats *st, const EpiPre<R> *pre = nullptr,
                                               DryDep<R> *defer = nullptr) {
  int itra1;
  if (nstop > 1) {
    itra1 = kDead;
    atomicAdd(&st->n_left, 1ull);
  } else {
    itra1 = itime + V.lsynctime;
    R xmassfract = (R)0;
    // release point of the particle: xmass(npoint(j),ks), npart(npoint(j)), timemanager.f90:663-666
    const bool massfract = V.mdomainfill == 0 && V.mquasilag == 0;
    // (with one release point every index into the point tables is clamped to it: npoint(j) is not needed, and the
    // table loads below do not wait for it)
    const int npoint = pre ? pre->npoint : ((massfract && V.numpoint > 1) || (DRYDEP && Gp.on)) ? P.npoint[s] : 1;
    const int kr = release_index(V, npoint);
    // everything the species loop reads -- the release point's table entries and the particle's masses -- in ONE round
    // trip (the asm ties the loads together; otherwise each is issued where it is first needed: three dependent trips)
    int npart_i = massfract ? V.rel_npart[kr] : 0;
    R xmr_all[kMaxSpec], xm_all[kMaxSpec];
#pragma unroll
    for (int ks = 0; ks < kMaxSpec; ks++) {
      xmr_all[ks] = (massfract && ks < V.nspec) ? V.rel_xmass[(size_t)ks * V.numpoint + kr] : (R)0;
      xm_all[ks] = ks < V.nspec ? ((pre && ks == 0) ? pre->xm0 : P.xmass1[(size_t)ks * P.cap + s]) : (R)0;
    }
    static_assert(kMaxSpec == 5, "the tie below names five species");
    asm volatile("" : "+v"(npart_i), "+v"(xmr_all[0]), "+v"(xmr_all[1]), "+v"(xmr_all[2]), "+v"(xmr_all[3]), "+v"(xmr_all[4]),
                      "+v"(xm_all[0]), "+v"(xm_all[1]), "+v"(xm_all[2]), "+v"(xm_all[3]), "+v"(xm_all[4]));
    const R npart_r = (R)npart_i;
#pragma unroll
    for (int ks = 0; ks < kMaxSpec; ks++) {
      if (ks < V.nspec) {
        R decfact = V.decay[ks] > (R)0 ? m_exp(-(R)abs(V.lsynctime) * V.decay[ks]) : (R)1;
        R xm = xm_all[ks];
        if (DRYDEP && V.drydepspec[ks]) {
          // timemanager.f90:650-656; drydeposit is real(dep_prec): 4 bytes in every build
          float drydeposit = (float)(xm * prob[ks] * decfact);
          xm = xm * ((R)1 - prob[ks]) * decfact;
          if (Gp.on && V.ldirect == 1) {   // timemanager.f90:690-696
            if (V.decay[ks] > (R)0) {
              const int ldeltat = itime < Gp.loutnext ? itime - (Gp.loutnext - Gp.loutstep) : itime - Gp.loutnext;   // :513-517
              drydeposit = (float)((R)drydeposit * m_exp((R)abs(ldeltat) * V.decay[ks]));
            }
            const int nage = ageclass(Gp, abs(itime - itramem));
            const int kp = Gp.ioutputforeachrelease == 1 ? npoint : 1;
            if (defer) {
              defer->dep[ks] = drydeposit; defer->x = (R)ps.xt; defer->y = (R)ps.yt; defer->nage = nage; defer->kp = kp; defer->nclass = P.nclass[s];
            } else {
              drydepo_particle(V, Gp, P.nclass[s], drydeposit, ks, (R)ps.xt, (R)ps.yt, nage, kp);
              if (Gp.nested) drydepo_particle(V, Gp, P.nclass[s], drydeposit, ks, (R)ps.xt, (R)ps.yt, nage, kp, true);   // timemanager.f90:694-696
            }
          }
        } else xm = xm * decfact;
        if (DRYDEP || V.decay[ks] > (R)0) P.xmass1[(size_t)ks * P.cap + s] = xm;
        if (massfract) {   // timemanager.f90:663-666
          const R xmr = xmr_all[ks];
          if (xmr > (R)0) xmassfract = m_max(xmassfract, npart_r * xm / xmr);
        } else {
          xmassfract = (R)1;
        }
      }
    }
    if (xmassfract < (R)0.0001) {   // minmass, par_mod.f90:213
      itra1 = kDead;
      atomicAdd(&st->n_minmass, 1ull);
    } else if (abs(itra1 - itramem) >= V.lage_last) {
      itra1 = kDead;
      atomicAdd(&st->n_maxage, 1ull);
    }
  }
  P.xt[s] = ps.xt; P.yt[s] = ps.yt; P.zt[s] = ps.zt;
  if (TURB) { P.up[s] = ps.up; P.vp[s] = ps.vp; P.cbt[s] = ps.icbt; }
  P.wp[s] = ps.wp;
  P.us[s] = ps.usigold; P.vs[s] = ps.vsigold; P.ws[s] = ps.wsigold;
  P.idt[s] = ps.ldt; P.itra1[s] = itra1;
}

// Per-slot hand-over record between the three PBL kernels: ONE contiguous, aligned record per particle (128 bytes in the
// fp64 build = one cache line, 64 bytes in f32), so that a lane that retires its particle in the Langevin kernel -- about
// two lanes of a wave per pass -- writes one line instead of a sector in each of sixteen arrays, and a refilling lane
// reads one.  k_prep fills the surface-layer part (FRESH), k_pbl_loop writes the particle's state at the end of its last
// pass (DONE / ESCAPED) -- or, when the launch's pass budget is used up (time slices, see k_pbl_loop), the state a later
// launch continues from (CONTINUE); k_pbl_finish reads it and writes the particle arrays, coalesced.
enum { PBL_FRESH = 3 };   // fourth value of the record's state next to PBL_CONTINUE / PBL_DONE / PBL_ESCAPED
template <typename R>
struct alignas(16 * sizeof(R)) PblRecord {
  // v[0..3]  = dxsave, dysave, dawsave, dcwsave                                  (CONTINUE, DONE, ESCAPED)
  // v[4..7]  = zt, up, vp, wp                                                    (CONTINUE, DONE, ESCAPED)
  // v[0..2]  = the step's invariants 1/ust | 1/ol, sigu, 1/tlu as StashInv holds them  (FRESH; read by the one-launch kernel only)
  // v[8..10] = ust, wst, ol (interpol_all.f90:80-107; ust as hanna.f90:43 floored it)  (FRESH, CONTINUE)
  //          | interpol_mod u, v, w of the last pass                             (DONE, ESCAPED)
  // v[11]    = CBL transition (cbl.f90:79-81), v[12] = mixing height of the cell (advance.f90:236-262): written by k_prep only
  // i[0] = nrand, i[1] = ldt, i[2] = state | icbt < 0 | indz | ngrid | |itimec - itime|  (pbl_pack)
  R v[13];
  int i[3];
};
static_assert(sizeof(PblRecord<double>) == 128 && sizeof(PblRecord<float>) == 64, "one cache line / half a line per record");
static_assert(sizeof(PblRecord<double>) == kRecStride * sizeof(double) && sizeof(PblRecord<float>) == kRecStride * sizeof(float) &&
              offsetof(PblRecord<double>, v) == 0 && offsetof(PblRecord<float>, v) == 0 && kRecWst < 13, "RecCold (fpx_device.hpp) indexes the records by these");
// state: bits 0-1, icbt = -1: bit 2, indz (<= 511): bits 3-11, ngrid + 2 (-2 .. kMaxNests): bits 12-14, |itimec - itime| (<= |lsynctime| <= 65535): bits 15-30
__device__ __forceinline__ int pbl_pack(int state, int icbt, int indz, int ngrid, int elapsed) {
  return state | (icbt < 0 ? 4 : 0) | (indz << 3) | ((ngrid + 2) << 12) | (elapsed << 15);
}
__device__ __forceinline__ int pbl_state(int pk) { return pk & 3; }
__device__ __forceinline__ int pbl_icbt(int pk) { return (pk & 4) ? -1 : 1; }
__device__ __forceinline__ int pbl_indz(int pk) { return (pk >> 3) & 511; }
__device__ __forceinline__ int pbl_ngrid(int pk) { return ((pk >> 12) & 7) - 2; }
__device__ __forceinline__ int pbl_elapsed(int pk) { return (pk >> 15) & 65535; }
static_assert(kMaxNz <= 512 && kMaxNests + 2 <= 7, "pbl_pack field widths");
template <typename R>
struct PblRec {
  PblRecord<R> *rec;       // [cap]
  R *tdep;                 // [cap], DRYDEP only: seconds of the step the particle spent below 2*href (advance.f90:582-599, see pbl_pass)
};

// Counters of the step's work list (unsigned ints, zeroed at the start of every step):
//   [0]     length of the whole list (all PBL particles; k_pbl_finish)
//   [kCtrBase + 12 j + ...]: launch j of the Langevin kernel (ONE pointer gives a launch everything it needs):
//     + c,     c = 0..3: particles of stability class c + 1 in its list (they sit at the head of the class's segment)
//     + 4 + c: the chunk cursor of that class
//     + 8 + c: first entry of the class's segment in the list (the list is sorted by class; the same in every launch)
constexpr int kMaxSlices = 16, kCtrBase = 8, kCtrStride = 12, kCtrWords = kCtrBase + (kMaxSlices + 1) * kCtrStride;

FPX_TU_CLOSE
}  // namespace fpx
