// k_prep, the first kernel of the particle step (timemanager.f90:531-712): every due particle -- initialize.f90 if it is
// newly released, the grid / cell / boundary-layer test of advance.f90:161-262; a particle above the boundary layer
// finishes its step here (interpol_wind + Petterssen, advance.f90:713-905), one inside it is set up (hanna, the hand-over
// record) and appended to the work list of k_pbl_loop.  prep_table maps a run's switches to the instance.
#pragma once
#include "fpx_step_common.hpp"

namespace fpx {
FPX_TU_OPEN

// Register budget: the steady-state kernel of a run on the mother lat-lon grid is built for FPX_PREP_WAVES waves per SIMD
// (<= 168 VGPRs, no scratch); the variants that also carry initialize(), the polar maps or the nest table would spill at
// that budget and keep two waves.
// The particle's step from the point where it is known to be due and inside the grid: initialize() if new, the boundary-layer
// test, the set-up of a boundary-layer particle or the whole step of one above it.  A function of its own so that k_prep can
// hold two instances: on a grid with polar caps (POLAR) the waves none of whose particles sits in a cap run the mother-grid
// instance (POLAR = false: compile-time ngrid = 0, field pointers in scalar registers, no stereographic code) with CAPCHECK
// (the test of advance.f90:843 still sees a particle that has moved INTO a cap); only the waves of the caps run the polar one.
template <typename R, bool DRYDEP, bool INIT, bool POLAR, bool NEST, bool CAPCHECK>
__device__ __forceinline__ void prep_body(const View<R> &V, const GridP<R> &Gp, Parts<R> &P, const SeqRng &S, const PblRec<R> &Q, long long s, int itime,
                                          unsigned int step, Stats *st, unsigned char *__restrict__ pbl_flag, const R *hgt,
                                          PState<R> &ps, int itramem, unsigned int pid) {
  constexpr bool MOTHER = !POLAR && !NEST;
  Rng<R> G;
  make_rng(V, pid, step, G);
  const bool is_new = INIT && ((itramem == itime) || (itime == 0));   // timemanager.f90:553
  if (is_new) {
    int nrand_i;
    R dcas = (R)0, dcas1 = (R)0;
    Rng<R> Gi = G;
    if (V.rng_mode == 0) {
      nrand_i = S.nrand_init[pid];
      if (sizeof(R) == 4) { dcas = (R)S.cbl_dcas[pid]; dcas1 = (R)S.cbl_dcas1[pid]; }
      else { dcas = (R)S.cbl_dcas_d[pid]; dcas1 = (R)S.cbl_dcas1_d[pid]; }
    } else {
      Gi.step = step | 0x80000000u;           // a stream of its own for initialize()
      nrand_i = V.rng_mode == 1 ? Gi.start_index(0) : 1;
      dcas = (R)(((float)(Gi.bits(1) >> 8) + 0.5f) * (1.0f / 16777216.0f));
      Rng<R> Gn = Gi;
      Gn.mode = 2;
      dcas1 = Gn.at(7);
    }
    initialize_particle(V, hgt, Gi, nrand_i, itime, ps, dcas, dcas1);
    atomicAdd(&st->n_init, 1ull);
  }

  AdvCtx<R> A;
  const TimeW<R> W = time_weights(V, itime);
  const bool in_pbl = adv_begin<R, MOTHER, true>(V, ps.xt, ps.yt, ps.zt, itime, advance_start_index(V, S, G, pid), A);
  if (V.lsettling) A.nsp = settling_species(V, P.npoint[s]);   // advance.f90:518-524 with nrelpoint = npoint(j)
  if (in_pbl) {
    if (is_new) {   // the PBL kernels read the state from HBM (an old particle's is there already)
      P.up[s] = ps.up; P.vp[s] = ps.vp; P.wp[s] = ps.wp;
      P.us[s] = ps.usigold; P.vs[s] = ps.vsigold; P.ws[s] = ps.wsigold;
      P.idt[s] = ps.ldt; P.cbt[s] = ps.icbt;
    }
    // first-pass set-up of interpol_all (ust, wst, ol: interpol_all.f90:80-107) done here, where
    // the lanes are convergent; the Langevin kernel then starts from five numbers per particle
    PblCtx<R> B;
    pbl_begin(V, ps.xt, ps.yt, W, A, B);
    // ... and what the turbulence scheme derives from them and the mixing height alone: fixed for the whole step, taken here
    // once instead of in each of the particle's 15 to 150 passes (step_invariants)
    const StepInv<R> I = step_invariants(A.h, B.ol, B.ust, B.wst, PlainMath());
    {
      PblRecord<R> &r = Q.rec[s];
      r.v[8] = I.ust; r.v[kRecWst] = B.wst; r.v[10] = B.ol; r.v[11] = B.transition;
      r.v[12] = A.h;
      r.v[0] = I.iaux; r.v[1] = I.sigu; r.v[2] = inv_pack_itlu(I);   // as the Langevin kernel's stash holds them (StashInv)
      // (the level of the particle's height travels with it: the Langevin kernel's first level search starts there, find_level_from)
      r.i[0] = A.nrand; r.i[2] = pbl_pack(PBL_FRESH, 1, find_level(hgt, V.nz, ps.zt), A.ngrid, 0);
    }
    // Regime class of the particle's PBL passes (hanna.f90:42,59,91 and advance.f90:405-406).  The
    // work list is the slots stably sorted by this 3-bit key: class by class, each class in slot
    // (= cell) order, so the lanes of a wave run the same branch of the turbulence scheme.
    unsigned char cls;
    if (V.cblflag == 1 && V.turbswitch && (I.flags & INV_DEEP)) cls = 1;      // skewed CBL scheme
    else if ((I.flags & INV_REGIME) == 0) cls = 3;                            // neutral
    else if ((I.flags & INV_REGIME) == 1) cls = 2;                                            // unstable, Gaussian: next to the CBL class, whose
                                                                              // hanna_short branch it shares (waves at a class boundary run both classes)
    else cls = 4;                                                             // stable
    // (measured and not kept: the reverse order -- 297.3 instead of 293.7 ms at 1e8, 47.9 instead of 42.2 ms at an eighth
    // of the cloud: the launch must not END on the CBL class, whose particles make the most passes; a cursor per class
    // with the waves dealt to the classes by their work -- 46.7 ms at an eighth: every class then ends at the end of the
    // launch; a cost bucket (octaves of (ustar+wstar)/h) below the class in the key: no measurable change)
    // Below the class: a cost bucket, the most expensive first.  The number of passes a particle makes is about |lsynctime| /
    // (its time step); its last time step of the previous step (idt) predicts that well where the time step is set by the
    // cell (ust, ol, h: the stable class keeps one value for the whole step).  With the long particles of a class at the head
    // of its segment, what the waves still hold when the cursor leaves the class -- and at the end of the launch -- are short
    // particles: less of the launch runs with half-empty or two-class waves.  Each bucket stays in slot (= cell) order.
    unsigned char bucket = 0;
    if (V.pbl_cost_buckets) {
      const int idt = is_new ? ps.ldt : P.idt[s];
      const int est = abs(V.lsynctime) / max(idt, 1);          // passes, if the time step stayed
      if (V.pbl_cost_buckets == 1) bucket = est >= 128 ? 3 : est >= 64 ? 2 : est >= 32 ? 1 : 0;
      else if (V.pbl_cost_buckets == 2) bucket = est >= 64 ? 1 : 0;
      else bucket = est >= 256 ? 7 : est >= 128 ? 6 : est >= 96 ? 5 : est >= 64 ? 4 : est >= 48 ? 3 : est >= 32 ? 2 : est >= 16 ? 1 : 0;
    }
    pbl_flag[s] = (unsigned char)((cls - 1) * 8 + (7 - bucket));
    return;
  }
  // Above the mixing layer for the whole step (advance.f90:629-708 -> 99): wp and ldt are set, not read; up, vp and cbt
  // are not touched; the mesoscale velocities are fetched with the last column of the 48-value gather (same round
  // trip, not live across the gather: the asm ties the loads to that point of the program).
  R usig, vsig, wsig;
  pbl_flag[s] = kKeyDone;
  auto late = [&]() {
    if (!is_new) {
      asm volatile("" : "+v"(s));
      ps.usigold = P.us[s]; ps.vsigold = P.vs[s]; ps.wsigold = P.ws[s];
    }
  };
  above_step<R, Rng<R>, true>(V, hgt, G, W, itime, ps.xt, ps.yt, ps.zt, ps.wp, ps.ldt, A, usig, vsig, wsig, late);
  // (fetching the epilogue's npoint / xmass1 with the Petterssen gather was tried here: the three registers spill at the
  // three-wave budget of this kernel; k_pbl_finish has them)
  const int nstop = adv_finish<R, Rng<R>, POLAR, MOTHER, NoLate, CAPCHECK>(V, hgt, G, itime, ps, A, usig, vsig, wsig);
  R prob[kMaxSpec];
#pragma unroll
  for (int ks = 0; ks < kMaxSpec; ks++) prob[ks] = (R)0;
  if (is_new) epilogue_store<R, DRYDEP, true>(V, Gp, P, s, itime, itramem, nstop, ps, prob, st);
  else epilogue_store<R, DRYDEP, false>(V, Gp, P, s, itime, itramem, nstop, ps, prob, st);
}

template <typename R, bool DRYDEP, bool INIT, bool POLAR, bool NEST>
__global__ void __launch_bounds__(kBlock, FPX_PREP_TWO_WAVES(INIT, POLAR, NEST, DRYDEP) ? 2 : FPX_PREP_WAVES) k_prep(View<R> V_arg, GridP<R> Gp_arg, Parts<R> P_arg, SeqRng S_arg, PblRec<R> Q_arg, long long numpart, int itime,
                                                 unsigned int step, Stats *st, unsigned char *__restrict__ pbl_flag,
                                                 unsigned int *__restrict__ pbl_count) {
#ifndef FPX_VIEW_BY_VALUE
  struct KArgs { View<R> V; GridP<R> Gp; Parts<R> P; SeqRng S; PblRec<R> Q; };   // the leading parameters as the segment holds them
  const KArgs &ka = *(const KArgs *)(const void *)__builtin_amdgcn_kernarg_segment_ptr();
  const View<R> &V = ka.V; const GridP<R> &Gp = ka.Gp; Parts<R> &P = const_cast<Parts<R> &>(ka.P); const SeqRng &S = ka.S; const PblRec<R> &Q = ka.Q;
  (void)V_arg; (void)Gp_arg; (void)P_arg; (void)S_arg; (void)Q_arg;
#else
  const View<R> &V = V_arg; const GridP<R> &Gp = Gp_arg; Parts<R> &P = P_arg; const SeqRng &S = S_arg; const PblRec<R> &Q = Q_arg;
#endif
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  __syncthreads();
  long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart) return;
  // the position travels in the same memory round trip as the due test (nearly every particle is due)
  PState<R> ps;
  const int itra1_in = P.itra1[s];
  ps.xt = P.xt[s]; ps.yt = P.yt[s]; ps.zt = P.zt[s];
  int itramem = P.itramem[s];
  unsigned int pid = P.pid[s];
  // ONE round trip: without this the compiler sinks each load into the branch that first needs it (itra1 -> wait -> xt ->
  // wait -> yt -> wait -> zt ...: five dependent round trips at the head of a latency-bound kernel)
  {
    int due_key = itra1_in;
    asm volatile("" : "+v"(due_key), "+v"(ps.xt), "+v"(ps.yt), "+v"(ps.zt), "+v"(itramem), "+v"(pid));
    if (due_key != itime) { pbl_flag[s] = kKeyNotDue; return; }    // timemanager.f90:537
  }
  // key kKeyNotDue = not due; kKeyDone = due, finished in this kernel (above the PBL); 8 (c - 1) + 0..7 = PBL particle of regime
  // class c = 1..4, cost bucket 7..0 (see below).
  // The counts (particles due, length of the PBL work list) are read off the sorted keys by
  // k_list_counts: one atomic per wave on a single address costs more than the whole kernel.

  // a non-finite or out-of-grid position would index outside the fields (the reference
  // would read arbitrary memory): terminate the particle instead
  if (!(ps.xt >= 0. && ps.xt <= (double)V.nxmin1 && ps.yt >= 0. && ps.yt <= (double)V.nymin1) || !(ps.zt == ps.zt)) {
    P.itra1[s] = kDead;
    pbl_flag[s] = kKeyDone;
    atomicAdd(&st->n_badpos, 1ull);
    return;
  }

  // wave-uniform: is any particle of this wave new (timemanager.f90:553)?  The INIT instance runs whenever particles MAY have
  // been released since the last step -- every step of a run with a continuous release -- but only the waves that do hold a
  // new particle need the body with initialize() in it (a dynamically indexed array in scratch, more registers); the others
  // run the steady-state body, so that the instance costs what the steady-state kernel costs.
  if (INIT && __any((itramem == itime) || (itime == 0))) {
    prep_body<R, DRYDEP, true, POLAR, NEST, false>(V, Gp, P, S, Q, s, itime, step, st, pbl_flag, hgt, ps, itramem, pid);
    return;
  }
  if (POLAR && !NEST) {
    // wave-uniform: does any particle of this wave start in a polar cap (advance.f90:161-164)?  The slots are cell-sorted, so
    // five waves in six of a global run do not
    if (!__any(pick_polar(V, ps.yt) != 0)) {
      prep_body<R, DRYDEP, false, false, false, true>(V, Gp, P, S, Q, s, itime, step, st, pbl_flag, hgt, ps, itramem, pid);
      return;
    }
  }
  prep_body<R, DRYDEP, false, POLAR, NEST, false>(V, Gp, P, S, Q, s, itime, step, st, pbl_flag, hgt, ps, itramem, pid);
}

FPX_TU_CLOSE
template <typename R>
static const void *prep_table(bool drydep, bool init, bool polar, bool nest) {
#define FPX_PREP(DD, II) (polar ? (nest ? (const void *)k_prep<R, DD, II, true, true> : (const void *)k_prep<R, DD, II, true, false>) \
                                : (nest ? (const void *)k_prep<R, DD, II, false, true> : (const void *)k_prep<R, DD, II, false, false>))
  if (drydep) return init ? FPX_PREP(true, true) : FPX_PREP(true, false);
  return init ? FPX_PREP(false, true) : FPX_PREP(false, false);
#undef FPX_PREP
}
}  // namespace fpx
