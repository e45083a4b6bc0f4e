// k_pbl_loop and k_pbl_finish, the second and third kernel of the particle step (timemanager.f90:531-712): the Langevin
// loop of advance.f90:264-611 for the boundary-layer particles of the work list (persistent waves, lane refill), and their
// completion, advance.f90:617-905 and the epilogue timemanager.f90:630-708.  loop_table and finish_table map a run's
// switches to the instance.
#pragma once
#include "../../include/flexpart_amd.h"
#include "fpx_step_common.hpp"

namespace fpx {
FPX_TU_OPEN

// The Langevin kernel: persistent waves, lane refill (see the comment on the hot kernels in fpx_step_common.hpp).
// Only the pass loop lives here; set-up and completion run in k_prep / k_pbl_finish
// where all lanes are active.
// LEAN: no dry deposition, no settling (gases).  TSW / CBLF / RNGM: see pbl_pass.
//
// The kernel runs as a short sequence of launches per step (Engine::step).  A lane can SUSPEND its particle between two
// passes: the state goes into the particle's hand-over record (state PBL_CONTINUE) and the slot is appended to the next
// launch's list, class by class (one atomic per wave and event); the next launch continues it.  Three rules, all decided
// per wave:
//  * class purity: the list is sorted by stability class, every class has a chunk cursor of its own and a wave draws from
//    ONE class at a time.  When that class has no chunk left the wave runs on with what it holds, without refilling,
//    until fewer than drain_lanes lanes are busy, suspends those particles and moves to the next class with all lanes
//    free -- so the lanes of a wave always run ONE branch of hanna_short / cbl (before: for up to 300 passes after the
//    cursor had crossed a class boundary the waves ran both classes' code for the sake of a few long-lived particles:
//    12 % of the hanna_short and 7 % of the CBL sub-steps at 1.25e7 particles);
//  * drain: the same rule after the last class -- the wave hands its last particles on and ends; the next launch packs
//    the leftovers of all waves densely (before: the last tenth of a launch ran with waves of a lane or two);
//  * pass budget (cap_passes > 0, optional): at most cap_passes passes per particle and launch.
// The last launch of the sequence has no next list (drain_lanes = 0, cap_passes = 0): it runs everything to the end.
// A particle's random numbers are keyed on (particle number, step, draw index) and the draw index travels in the record:
// suspending does not change a bit of the result (tests/test_gpu_parity.py::test_time_slices_do_not_change_a_bit).
// SUSP = false: the instance of a step with ONE launch -- nothing can be suspended or resumed, and the refill, which runs with two
// lanes of the wave, carries none of that (the hand-over of suspended particles cost 2 % of the kernel's instructions at 1e8).
template <typename R, bool LEAN, int TSW, int CBLF, int RNGM, bool SUSP = false>
__global__ void __launch_bounds__(kBlock, sizeof(R) == 4 ? FPX_LOOP_WAVES_F32 : FPX_LOOP_WAVES) k_pbl_loop(View<R> V_arg, Parts<R> P_arg, PblRec<R> Q_arg, int itime, unsigned int step, Stats *st,
                                                     const unsigned int *__restrict__ pbl_list,
                                                     unsigned int *__restrict__ blk,
                                                     int cap_passes, int drain_lanes,
                                                     unsigned int *__restrict__ next_list) {
  // (the View alone: k_pbl_loop<double, true, 1, 1, 2> 157 -> 153 VGPRs, 49 -> 19 spilled SGPRs, 24 B -> no scratch; -0.5 to -1 % of the launch)
#if !defined(FPX_VIEW_BY_VALUE) && !defined(FPX_LOOP_ONLY_VIEW)
  struct KArgs { View<R> V; Parts<R> P; PblRec<R> Q; };
  const KArgs &ka = *(const KArgs *)(const void *)__builtin_amdgcn_kernarg_segment_ptr();
  const View<R> &V = ka.V; const Parts<R> &P = ka.P; const PblRec<R> &Q = ka.Q;
  (void)V_arg; (void)P_arg; (void)Q_arg;
#else
  FPX_VIEW_FROM_KERNARG(V, V_arg);
  const Parts<R> &P = P_arg; const PblRec<R> &Q = Q_arg;
#endif
  // blk: this launch's block of the counters (see k_list_counts): per class c the first blk[c] entries of the class's segment
  // [blk[8 + c], ...) of pbl_list, the class's chunk cursor blk[4 + c]; the next launch's block follows
  const unsigned int *mine = blk;
  unsigned int *next_cnt = blk + kCtrStride;
  // (only the current class's length and segment start live in scalar registers, not all four: twelve registers through the
  // whole kernel were taken from the polynomial constants of the fine loop, which then came back through v_readlane in
  // every sub-step)
  // A short list (the later launches): only as many blocks as it fills take part, so that its waves are spread over the
  // CUs one block each instead of three to a SIMD on some and none on others (a pass of a wave alone on its SIMD takes a
  // third of the time).
  const unsigned int nlist_all = mine[0] + mine[1] + mine[2] + mine[3];
  if ((unsigned long long)blockIdx.x * kBlock >= (unsigned long long)nlist_all) return;
  const bool can_suspend = SUSP && (drain_lanes > 0 || cap_passes > 0);
  // dynamic LDS: [S_COUNT][kBlock] stash (per-lane pass-level state, see Stash) + the height column,
  // sized by the host (loop_smem_bytes) so that three blocks fit one CU for the usual nz
  extern __shared__ __align__(16) unsigned char fpx_loop_smem[];
  static_assert(kStashStride == kBlock, "stash layout is one column per thread of the block");
  R *stash_mem = reinterpret_cast<R *>(fpx_loop_smem);
  R *hgt = stash_mem + stash_slots<R>(LEAN, SUSP) * kStashStride;   // (the host sizes the block's LDS alike: loop_smem_bytes)
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  // the block's copy of the lookup tables of the fp64 logarithm and exponential (m_log_abs, m_exp_tab): 768 B
  // ... and, where the block has the room (the fp64 gas kernels), of the 256-entry table of the exponential in place of the
  // 32-entry one (2.5 KB with the logarithm's) and of the table of the error-function pair (m_erf_tab2, 8.1 KB): static like
  // the tables above, so the host's rule for the dynamic part (loop_smem_bytes) does not change.  With them a one-launch fp64
  // gas kernel has 19 x 2 KB + 8 nz + 10880 B per block: 50896 B at nz = 138, three blocks per CU (53248 B each) up to
  // nz = 432; its time-sliced twin (20 slots) 52944 B, three up to nz = 176 (kLdsGasStaticBytes in fpx_device.hpp).
  constexpr bool ERFTAB = stash_has_erf_tab<R>(LEAN);
  constexpr bool EXPFINE = ERFTAB && FPX_EXP_TAB_FINE != 0;
  __shared__ double lds_tab[sizeof(R) == 8 ? lds_tab_doubles(EXPFINE) : 1];
  if (EXPFINE) lds_tab_fill_fine(lds_tab);
  else if (sizeof(R) == 8)
    for (int k = threadIdx.x; k < kLdsTabDoubles; k += blockDim.x) lds_tab[k] = k < kLdsExpTabAt ? kLogTab[k >> 1][k & 1] : kExpTab[k - kLdsExpTabAt];
  __shared__ __align__(16) double lds_erft[ERFTAB ? kErfcxIntervals * kErfcxRow : 2];
  if (ERFTAB)
    for (int k = threadIdx.x; k < kErfcxIntervals * kErfcxRow; k += blockDim.x) lds_erft[k] = kErfcxTab[k];
  __syncthreads();
  typedef typename StashFor<R, ERFTAB>::type stash_t;
  const stash_t S = make_stash<R, ERFTAB>((typename Stash<R>::lds_ptr)(stash_mem + threadIdx.x), (lds_tab_ptr)lds_tab, (lds_erft_ptr)lds_erft);
  const int lane = threadIdx.x & 63;
  const TimeW<R> W = time_weights(V, itime);   // wave-uniform
  const R cap_r = cap_passes > 0 ? (R)cap_passes : (R)1e30;

  // The list is in slot order, i.e. sorted by grid cell after a locality sort.  A wave takes
  // CHUNKS of consecutive entries (one atomic per chunk) and refills its lanes from its own
  // chunk, so the particles a wave works on at any moment come from neighbouring cells
  // (same mixing height, same stability regime, shared cache lines).
  // 64 entries per claim: with larger chunks (nlist/(8*nwaves) = 2000 entries at 1e8 was tried first) the kernel
  // ended half a chunk's worth of work -- tens of milliseconds -- after the list ran out, most waves idle;
  // measured 429 -> 395 ms.  One atomic per 64 refills is still negligible.
  unsigned int cur = 0, end = 0;     // wave-uniform: the unread part of the wave's chunk
  unsigned int cbase = 0;            // wave-uniform: first entry of the chunk
  unsigned int ahead = 0;            // lane l: entry cbase + l of the list (the whole chunk, read with the claim)
  bool out_of_chunks = false;        // wave-uniform
  int wcls = 0;                      // wave-uniform: class (0..3) the wave draws its particles from
  unsigned int cls_out = 0u;         // wave-uniform: that class has no chunk left
  unsigned int cls_n = mine[0], cls_seg = mine[8];   // wave-uniform: length and first entry of that class's segment (read again when the wave moves on)
  // The wave-uniform values that are only read where a chunk is claimed -- once per 64 particles -- are kept in VECTOR
  // registers (the kernel has nine to spare; the empty asm makes them lane values for the compiler), not in scalar ones: the
  // scalar file is what the fine loop's polynomial constants live in, and every scalar held across the loop came back as a
  // v_readlane in each sub-step (+0.8 % VALU instructions at 1e8 with all of these in scalar registers).
#define FPX_IN_VGPR(x) asm volatile("" : "+v"(x))
  if (SUSP) { FPX_IN_VGPR(cbase); FPX_IN_VGPR(cls_out); FPX_IN_VGPR(cls_n); FPX_IN_VGPR(cls_seg); }
#ifdef FPX_LANE_STATS
  const unsigned long long t_s = wall_clock64();   // 100 MHz; timeline of the wave: start, list exhausted, end
  unsigned long long t_x = 0;
#endif

  bool have = false;
  unsigned int s = 0, pid = 0;
  double xt = 0, yt = 0;
  R zt = 0, wp = 0;
  int ldt = 0;
  short icbt = 1;
  int lvl = 0;                       // the level of the lane's last pass, where the next pass starts its level search (find_level_from); 0: none
  LoopCtx<R> A;

  // the lanes of `who` (all of them hold a particle) hand their particles on: record written, slot appended to the next
  // launch's list in the segment of the wave's class
  auto write_record = [&](int state, int indz) {
    PblRecord<R> *rp = Q.rec + s;
    rp->v[0] = S.get(S_DX); rp->v[1] = S.get(S_DY); rp->v[2] = S.get(S_DAW); rp->v[3] = S.get(S_DCW);
    rp->v[4] = zt; rp->v[5] = S.get(S_UP); rp->v[6] = S.get(S_VP); rp->v[7] = wp;
    if (state == PBL_CONTINUE) {
      rp->v[8] = S.get(S_UST);      // hanna.f90:43 may have floored it; v[9..12] stay as k_prep wrote them
    } else {
      rp->v[8] = S.get(S_U); rp->v[9] = S.get(S_V); rp->v[10] = S.get(S_W);
    }
    rp->i[0] = A.nrand; rp->i[1] = ldt;
    rp->i[2] = pbl_pack(state, icbt, indz, A.ngrid, abs(A.itimec - itime));
    if (!LEAN && V.drydep) Q.tdep[s] = S.get(S_TDEP);
  };
  auto suspend = [&](bool mine_goes) {   // convergent: every lane of the wave calls it
    const unsigned long long sm = __ballot(mine_goes);
    if (sm == 0ull) return;
    if (mine_goes) { write_record(PBL_CONTINUE, lvl); have = false; }
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(next_cnt + wcls, (unsigned int)__popcll(sm));
    base = __builtin_amdgcn_readfirstlane(base);
    const unsigned int seg = mine[8 + wcls];
    if (mine_goes) next_list[seg + base + (unsigned int)__popcll(sm & ((1ull << lane) - 1ull))] = s;
  };

  for (;;) {
    FPX_LANES(st, 10);
    unsigned long long need = __ballot(!have);
    if (need != 0ull && !out_of_chunks) {
      if (!SUSP) {
        // One launch, nothing to suspend: the class segments of the list are adjacent, so the wave walks the list as ONE
        // sequence with ONE cursor (chunks may straddle a class boundary, as in round 3)
        if (cur >= end) {
          unsigned int c = 0;
          if (lane == 0) c = atomicAdd(blk + 4, 1u);
          c = __builtin_amdgcn_readfirstlane(c);
          const unsigned long long c0 = (unsigned long long)c * 64u;
          if (c0 >= nlist_all) {
            out_of_chunks = true;
#ifdef FPX_LANE_STATS
            t_x = wall_clock64();
#endif
          } else {
            cur = (unsigned int)c0;
            cbase = cur;
            end = min(cur + 64u, nlist_all);
            ahead = pbl_list[min(cur + (unsigned int)lane, nlist_all - 1u)];
          }
        }
      } else
      while (cur >= end && !out_of_chunks) {   // wave-uniform: take the next chunk of the wave's class
        if (__builtin_amdgcn_readfirstlane(cls_out) == 0u) {
          const unsigned int nseg = __builtin_amdgcn_readfirstlane(cls_n), seg = __builtin_amdgcn_readfirstlane(cls_seg);
          const unsigned int kk = (nseg + 63u) >> 6;       // this class's length in chunks
          unsigned int c = 0;
          if (lane == 0) c = atomicAdd(blk + 4 + wcls, 1u);
          c = __builtin_amdgcn_readfirstlane(c);
          if (c < kk) {
            cur = seg + c * 64u;
            cbase = cur; FPX_IN_VGPR(cbase);
            end = min(cur + 64u, seg + nseg);
            ahead = pbl_list[min(cur + (unsigned int)lane, end - 1u)];
            break;
          }
          cls_out = 1u; FPX_IN_VGPR(cls_out);
        }
        // The wave's class has no chunk left.  A launch that can hand particles on keeps the wave on what it holds -- no
        // refill, so no second class in the wave -- until fewer than drain_lanes lanes are busy, then suspends those and
        // moves on to the next class with all lanes free; the last launch moves on at once (and mixes).
        if (can_suspend) {
          const int live = __popcll(__ballot(have));
          if (live > 0 && live >= drain_lanes) break;
          suspend(have);
          need = ~0ull;
        }
        wcls++;
        cls_out = 0u; FPX_IN_VGPR(cls_out);
        if (wcls < 4) { cls_n = mine[wcls]; cls_seg = mine[8 + wcls]; FPX_IN_VGPR(cls_n); FPX_IN_VGPR(cls_seg); }
        if (wcls == 4) {
          out_of_chunks = true;
#ifdef FPX_LANE_STATS
          t_x = wall_clock64();
#endif
        }
      }
      if (cur < end) {
        // A refill is ONE memory round trip: the list entry comes from the chunk read above (cross-lane), everything else
        // depends on the slot only and is requested together -- grid and mixing height travel in the record k_prep wrote.
        // (Before: list entry -> state -> mixing height -> six stash values one after the other = nine dependent round
        // trips, with two of the wave's lanes active, in 60 % of the passes.)
        const unsigned int rank = __popcll(need & ((1ull << lane) - 1ull));
        const unsigned int my = cur + rank;
        const unsigned int s_new = (unsigned int)__builtin_amdgcn_ds_bpermute((int)(min(my - cbase, 63u) << 2), (int)ahead);   // all lanes
        if (!have && my < end) {
          FPX_LANES(st, 8);
          s = s_new;
          const PblRecord<R> *rp = Q.rec + s;
          const double l_xt = P.xt[s], l_yt = P.yt[s];
          const unsigned int l_pid = P.pid[s];
          const int r_nrand = rp->i[0], r_ldt = SUSP ? rp->i[1] : 0, r_pk = rp->i[2];
          const R r_ust = rp->v[8], r_wst = rp->v[kRecWst], r_ol = rp->v[10], r_trans = rp->v[11], r_h = rp->v[12];
          // the step's invariants as k_prep took them, same line as the above (a launch that may meet a suspended particle, whose
          // v[0..7] are in use, takes them here instead: step_invariants below)
          const R r_iaux = SUSP ? (R)0 : rp->v[0], r_sigu = SUSP ? (R)0 : rp->v[1], r_itlu = SUSP ? (R)0 : rp->v[2];
          // a fresh particle's state is in the particle arrays, a suspended one's in its record: both are requested
          // (one round trip either way; suspended particles are the few)
          R l_zt = P.zt[s], l_wp = P.wp[s], l_up = P.up[s], l_vp = P.vp[s];
          int l_idt = P.idt[s];
          short l_cbt = P.cbt[s];
          const R c_dx = SUSP ? rp->v[0] : (R)0, c_dy = SUSP ? rp->v[1] : (R)0, c_daw = SUSP ? rp->v[2] : (R)0, c_dcw = SUSP ? rp->v[3] : (R)0;
          const R c_zt = SUSP ? rp->v[4] : (R)0, c_up = SUSP ? rp->v[5] : (R)0, c_vp = SUSP ? rp->v[6] : (R)0, c_wp = SUSP ? rp->v[7] : (R)0;
          int l_npoint = 0;
          if (!LEAN && V.lsettling) l_npoint = P.npoint[s];
          R c_tdep = (R)0;
          if (SUSP && !LEAN && V.drydep) c_tdep = Q.tdep[s];
          __builtin_amdgcn_sched_barrier(0);   // every load above is issued before the first value is used
          const bool resumed = SUSP && pbl_state(r_pk) == PBL_CONTINUE;
          xt = l_xt; yt = l_yt; pid = l_pid;
          zt = resumed ? c_zt : l_zt; wp = resumed ? c_wp : l_wp;
          ldt = resumed ? r_ldt : l_idt;
          icbt = resumed ? (short)pbl_icbt(r_pk) : l_cbt;
          lvl = pbl_indz(r_pk);   // k_prep's level of the particle's height (FRESH), or that of its last pass (CONTINUE): a guess, tested before use
          {
            R ddx, ddy;
            adv_begin_known(V, xt, yt, pbl_ngrid(r_pk), r_h, A, ddx, ddy);
            A.itimec = SUSP ? itime + pbl_elapsed(r_pk) * V.ldirect : itime;   // FRESH: elapsed = 0
            A.nrand = r_nrand;
            A.nsp = 0;
            if (!LEAN && V.lsettling) {
              const int nsp = settling_species(V, l_npoint);
              const SettleSpec<R> sp = settle_spec(V, nsp);
              S.put(S_SET_NUM, spec_row(V, nsp).density > (R)0 ? sp.num : (R)0);   // density(nsp) <= 0: no settling (advance.f90:525)
              S.put(S_SET_DQ6, sp.dq6); S.put(S_SET_V0, sp.vset);
              S.put(S_SETCELL, (R)settling_column(V, (R)xt, (R)yt));   // < nx*ny: exact in R (f32: grids up to 2^24 columns, checked at fpx_create)
              if (sizeof(R) == 4) S.put(S_RT_TAG, (R)0);
            }
            S.put(S_DDX, ddx); S.put(S_DDY, ddy);
          }
          S.put(S_DX, resumed ? c_dx : (R)0); S.put(S_DY, resumed ? c_dy : (R)0);
          S.put(S_DAW, resumed ? c_daw : (R)0); S.put(S_DCW, resumed ? c_dcw : (R)0);
          S.put(S_W, (R)0);
          S.put(S_UP, resumed ? c_up : l_up); S.put(S_VP, resumed ? c_vp : l_vp);
          S.put(S_WST2, r_wst * r_wst);
          S.put(S_OL, r_ol);
          S.put(S_TRANS, (r_wst * r_wst * r_wst) * r_trans);   // (wst**3)*transition, cbl.f90:103-104
          if (SUSP) S.put(S_NPASS, (R)0);
          if (!LEAN && V.drydep) S.put(S_TDEP, resumed ? c_tdep : (R)0);
          if (SUSP) {
            __builtin_amdgcn_sched_barrier(0);   // last, with everything else of the refill stored: the helper's temporaries do not meet the loaded values
            const StepInv<R> I = step_invariants(r_h, r_ol, r_ust, r_wst, S);
            S.put(S_UST, I.ust); S.put(S_IAUX, I.iaux); S.put(S_SIGU, I.sigu); S.put(S_ITLU, inv_pack_itlu(I));
          } else {
            S.put(S_UST, r_ust); S.put(S_IAUX, r_iaux); S.put(S_SIGU, r_sigu); S.put(S_ITLU, r_itlu);
          }
          have = true;
        }
        cur = min(cur + (unsigned int)__popcll(need), end);
      }
    }
    if (!__any(have)) {
      if (out_of_chunks) break;   // no lane has work and the list is used up: the grid drains
      continue;                   // chunk ran dry mid-refill: take the next one
    }
    bool over_budget = false;
    if (have) {
      Rng<R, RNGM> G;
      make_rng(V, pid, step, G);
      const int rc = pbl_pass<R, !LEAN, !LEAN, TSW, CBLF>(V, hgt, G, W, itime, xt, yt, zt, wp, ldt, icbt, A, S, lvl, st, RecCold<R>{Q.rec[0].v, s});
      R npass = (R)0;
      if (SUSP) { npass = S.get(S_NPASS) + (R)1; S.put(S_NPASS, npass); }
      if (rc != PBL_CONTINUE) {
        FPX_LANES(st, 9);
        // the particle's state at the end of its last pass goes into its hand-over record: one contiguous line;
        // k_pbl_finish writes the particle arrays from it
        write_record(rc, lvl);
        have = false;
      } else over_budget = SUSP && npass >= cap_r;
    }
    if (SUSP && cap_passes > 0) suspend(over_budget);
  }
#ifdef FPX_LANE_STATS
  if (lane == 0) {
    const unsigned long long t_e = wall_clock64();
    atomicAdd(&st->lanes[11][0], 1ull);
    atomicAdd(&st->lanes[11][1], t_x - t_s);            // sum over waves: start -> list exhausted
    atomicAdd(&st->lanes[12][0], t_e - t_s);            // sum over waves: start -> end
    atomicMax(&st->lanes[12][1], t_e - t_s);            // longest wave
    atomicMax(&st->lanes[13][0], ~(t_x - t_s));         // ~(first wave to see the list exhausted)
    atomicMax(&st->lanes[13][1], t_e - t_x);            // longest drain of one wave
  }
#endif
}

// completion of ONE boundary-layer particle: label 700 if it left the PBL, sigmas for the mesoscale term, label 99 to the end
// of advance(), epilogue.  A function of its own for the same reason as prep_body: on a grid with polar caps the waves without
// a particle in a cap run the mother-grid instance (POLAR = false, CAPCHECK), the others the polar one.
template <typename R, bool DRYDEP, bool POLAR, bool NEST, bool CAPCHECK>
__device__ __forceinline__ void finish_body(const View<R> &V, const GridP<R> &Gp, Parts<R> &P, unsigned int s, const PblRecord<R> &rec, R tdep,
                                            int itime, unsigned int step, Stats *st, const R *hgt, DryDep<R> *dry) {
  constexpr bool MOTHER = !POLAR && !NEST;
  const int pk = rec.i[2];
  PState<R> ps;
  ps.xt = P.xt[s]; ps.yt = P.yt[s]; ps.zt = rec.v[4];
  ps.up = rec.v[5]; ps.vp = rec.v[6]; ps.wp = rec.v[7];
  ps.usigold = P.us[s]; ps.vsigold = P.vs[s]; ps.wsigold = P.ws[s];
  ps.ldt = rec.i[1]; ps.icbt = (short)pbl_icbt(pk);
  Rng<R> G;
  make_rng(V, P.pid[s], step, G);
  const TimeW<R> W = time_weights(V, itime);
  AdvCtx<R> A;
  {
    // same cell as at entry: the horizontal position does not change inside the loop
    AdvCtx<R> A0;
    adv_begin<R, MOTHER>(V, ps.xt, ps.yt, ps.zt, itime, 0, A0);
    A = A0;
  }
  if (V.lsettling) A.nsp = settling_species(V, P.npoint[s]);
  A.dxsave = rec.v[0]; A.dysave = rec.v[1]; A.dawsave = rec.v[2]; A.dcwsave = rec.v[3];
  A.u = rec.v[8]; A.v = rec.v[9]; A.w = rec.v[10];
  A.nrand = rec.i[0]; A.itimec = itime + pbl_elapsed(pk) * V.ldirect;
  const int rc = pbl_state(pk), indz = pbl_indz(pk);   // (every particle of the list is DONE or ESCAPED when the last time slice has run)
  R usig = (R)0, vsig = (R)0, wsig = (R)0;
  R prob[kMaxSpec];
  {
    Cell<R> C;
    cell_setup(C, A.ix, A.jy, A.ixp, A.jyp, A.xr, A.yr);
    if (rc == PBL_ESCAPED) {
      above_step(V, hgt, G, W, itime, ps.xt, ps.yt, ps.zt, ps.wp, ps.ldt, A, usig, vsig, wsig);
    } else {
      level_pair_sigma(V, fld_of(V, A.ngrid), C, W, indz, usig, vsig, wsig);   // advance.f90:604-606
    }
    // advance.f90:582-599 in closed form: prob(ks) = 1 - exp(-vdepo(ks) * T / (2*href)), T = the loop's sum of |dt| over the
    // passes that ended below 2*href (pbl_pass); the deposition velocity of the particle's cell, as every pass saw it
#pragma unroll
    for (int ks = 0; ks < kMaxSpec; ks++) {
      prob[ks] = (R)0;
      if (DRYDEP && ks < V.nspec && V.drydepspec[ks]) {
        const R vdepo = interp_vdep(V, fld_of(V, A.ngrid), C, W, ks);
        prob[ks] = (R)1 - m_expp(-vdepo * tdep / ((R)2. * (R)15.));   // href = 15, par_mod.f90:76
      }
    }
  }
  // what the epilogue reads of the particle travels with the last gather
  EpiPre<R> pre;
  int itramem = 0;
  unsigned int sl = s;
  auto late_epi = [&]() {
    asm volatile("" : "+v"(sl));
    pre.template load<DRYDEP>(V, Gp, P, sl);
    itramem = P.itramem[sl];
  };
  const int nstop = adv_finish<R, Rng<R>, POLAR, MOTHER, decltype(late_epi), CAPCHECK>(V, hgt, G, itime, ps, A, usig, vsig, wsig, late_epi);
  epilogue_store<R, DRYDEP>(V, Gp, P, s, itime, itramem, nstop, ps, prob, st, &pre, dry);
}

// completion of the PBL particles (finish_body).  One thread per list entry or slot.
template <typename R, bool DRYDEP, bool POLAR, bool NEST>
__global__ void __launch_bounds__(kBlock, FPX_FINISH_WAVES) k_pbl_finish(View<R> V_arg, GridP<R> Gp_arg, Parts<R> P_arg, PblRec<R> Q_arg, int itime, unsigned int step, Stats *st,
                                                       const unsigned char *__restrict__ pbl_key, long long numpart,
                                                       const unsigned int *__restrict__ pbl_list, const unsigned int *__restrict__ pbl_count) {
#ifndef FPX_VIEW_BY_VALUE
  struct KArgs { View<R> V; GridP<R> Gp; Parts<R> P; PblRec<R> Q; };
  const KArgs &ka = *(const KArgs *)(const void *)__builtin_amdgcn_kernarg_segment_ptr();
  const View<R> &V = ka.V; const GridP<R> &Gp = ka.Gp; Parts<R> &P = const_cast<Parts<R> &>(ka.P); const PblRec<R> &Q = ka.Q;
  (void)V_arg; (void)Gp_arg; (void)P_arg; (void)Q_arg;
#else
  const View<R> &V = V_arg; const GridP<R> &Gp = Gp_arg; Parts<R> &P = P_arg; const PblRec<R> &Q = Q_arg;
#endif
  // Two orders.  pbl_list given: the work list (class by class, each class in slot = cell order): every lane busy.  With cost
  // buckets in the list (32 interleaved sub-sequences of the cell-sorted slots) following it costs this kernel half of its
  // time again in scattered record and state accesses (0.58 -> 0.87 ms at 1.25e7 particles); then pbl_list is null and the
  // kernel goes through the SLOTS, taking those whose key of this step says "boundary layer" (0.77 ms when every slot has a
  // lane and the others idle; with the per-wave queue below the waves are full).
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  __syncthreads();
  // Slot order: every wave walks tiles of 64 consecutive slots, collects the boundary-layer ones in a queue of its own in LDS
  // and works them off 64 at a time -- full waves in (nearly) slot order, whatever share of a tile is boundary layer.
  __shared__ unsigned int queue_mem[kBlock / 64][128];
  // (an LDS pointer by type: as a generic one it made the compiler emit an instruction its own verifier rejects in the polar instance)
  typedef volatile unsigned int __attribute__((address_space(3))) *lds_queue_ptr;
  const lds_queue_ptr queue = (lds_queue_ptr)&queue_mem[threadIdx.x >> 6][0];
  const int lane = threadIdx.x & 63;
  unsigned int qlen = 0;   // wave-uniform
  const long long nwork = pbl_list ? (long long)*pbl_count : (numpart + 63) >> 6;   // list entries | tiles of 64 slots
  const long long stride = pbl_list ? (long long)gridDim.x * blockDim.x : (long long)gridDim.x * (kBlock / 64);
  long long it = pbl_list ? (long long)blockIdx.x * blockDim.x : (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  for (;;) {   // ONE body for both orders (the body is large: a single call site keeps it inlined once)
    // one wave's worth of particles: slot s for the lanes with `mine` (every lane of the wave goes through the body: the
    // dry-deposition scatter at its end needs them all)
    unsigned int s = 0;
    bool mine = false;
    if (pbl_list) {
      if (it >= nwork) break;          // the same for every lane of the block
      const long long i = it + threadIdx.x;
      mine = i < nwork;
      if (mine) s = pbl_list[i];
      it += stride;
    } else {
      while (qlen < 64u && it < nwork) {
        const long long i = it * 64 + lane;
        const bool pbl = i < numpart && pbl_key[i] < kKeyDone;
        const unsigned long long m = __ballot(pbl);
        if (pbl) queue[qlen + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = (unsigned int)i;
        qlen += (unsigned int)__popcll(m);
        it += stride;
      }
      if (qlen == 0u) break;           // the same for every lane of the wave
      const unsigned int take = min(qlen, 64u), rest = qlen - take;
      mine = (unsigned int)lane < take;
      if (mine) s = queue[lane];
      const unsigned int carry = (unsigned int)lane < rest ? queue[64 + lane] : 0u;
      if ((unsigned int)lane < rest) queue[lane] = carry;
      qlen = rest;
    }
    DryDep<R> dry;
#pragma unroll
    for (int ks = 0; ks < kMaxSpec; ks++) dry.dep[ks] = 0.f;
    dry.x = (R)0; dry.y = (R)0; dry.nage = 1; dry.kp = 1; dry.nclass = 1;
    if (mine) {
      const PblRecord<R> rec = Q.rec[s];
      const R tdep = DRYDEP ? Q.tdep[s] : (R)0;
      if (POLAR && !NEST && !__any(pbl_ngrid(rec.i[2]) < 0)) {   // wave-uniform: no particle of this wave sits in a polar cap
        finish_body<R, DRYDEP, false, false, true>(V, Gp, P, s, rec, tdep, itime, step, st, hgt, DRYDEP ? &dry : nullptr);
      } else {
        finish_body<R, DRYDEP, POLAR, NEST, false>(V, Gp, P, s, rec, tdep, itime, step, st, hgt, DRYDEP ? &dry : nullptr);
      }
    }
    if (DRYDEP && Gp.on && V.ldirect == 1) {
      // drydepokernel / drydepokernel_nest (timemanager.f90:690-696), with every lane of the wave: lanes of the same output
      // cell are summed into its neighbourhood before the atomics (wave_kernel_add); a lane without a deposit adds nothing
#pragma unroll
      for (int ks = 0; ks < kMaxSpec; ks++) {
        if (ks < V.nspec && V.drydepspec[ks]) {
          drydepo_particle<R, true>(V, Gp, dry.nclass, dry.dep[ks], ks, dry.x, dry.y, dry.nage, dry.kp);
          if (Gp.nested) drydepo_particle<R, true>(V, Gp, dry.nclass, dry.dep[ks], ks, dry.x, dry.y, dry.nage, dry.kp, true);
        }
      }
    }
  }
}

FPX_TU_CLOSE
// the Langevin kernel specialised for the run's switches (gases: LEAN) or the general one
template <typename R, bool SUSP>
static const void *loop_table_s(bool lean, int turbswitch, int cblflag, int rng_mode, bool *is_lean) {
  const bool philox = rng_mode == FPX_RNG_PHILOX;
  *is_lean = false;
  if (turbswitch < 0) return (const void *)k_pbl_loop<R, false, -1, -1, -1, SUSP>;   // turboff: the general instance (it alone has the switch)
  if (lean) {
    *is_lean = true;
    if (turbswitch && cblflag == 1) return philox ? (const void *)k_pbl_loop<R, true, 1, 1, 2, SUSP> : (const void *)k_pbl_loop<R, true, 1, 1, 0, SUSP>;
    if (turbswitch && cblflag != 1) return philox ? (const void *)k_pbl_loop<R, true, 1, 0, 2, SUSP> : (const void *)k_pbl_loop<R, true, 1, 0, 0, SUSP>;
    if (!turbswitch && cblflag != 1) return philox ? (const void *)k_pbl_loop<R, true, 0, 0, 2, SUSP> : (const void *)k_pbl_loop<R, true, 0, 0, 0, SUSP>;
    *is_lean = false;
  } else if (philox) {   // aerosols (settling / dry deposition) with the counter RNG: same switch specialisation
    if (turbswitch && cblflag == 1) return (const void *)k_pbl_loop<R, false, 1, 1, 2, SUSP>;
    if (turbswitch && cblflag != 1) return (const void *)k_pbl_loop<R, false, 1, 0, 2, SUSP>;
  }
  return (const void *)k_pbl_loop<R, false, -1, -1, -1, SUSP>;
}
// (a step of several launches runs the SUSP twin of the SAME specialisation: the arithmetic of a particle must not depend on
// how its step is scheduled -- two instances with different compile-time switches round differently)
template <typename R>
static const void *loop_table(bool lean, int turbswitch, int cblflag, int rng_mode, bool susp, bool *is_lean) {
  return susp ? loop_table_s<R, true>(lean, turbswitch, cblflag, rng_mode, is_lean) : loop_table_s<R, false>(lean, turbswitch, cblflag, rng_mode, is_lean);
}
template <typename R>
static const void *finish_table(bool drydep, bool polar, bool nest) {
  if (drydep) return polar ? (nest ? (const void *)k_pbl_finish<R, true, true, true> : (const void *)k_pbl_finish<R, true, true, false>)
                           : (nest ? (const void *)k_pbl_finish<R, true, false, true> : (const void *)k_pbl_finish<R, true, false, false>);
  return polar ? (nest ? (const void *)k_pbl_finish<R, false, true, true> : (const void *)k_pbl_finish<R, false, true, false>)
               : (nest ? (const void *)k_pbl_finish<R, false, false, true> : (const void *)k_pbl_finish<R, false, false, false>);
}
}  // namespace fpx
