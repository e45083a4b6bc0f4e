// The output grid: sampling of the particles (conccalc.f90:50-295), the receptor block of backward deposition runs
// (timemanager.f90:564-598, get_vdep_prob.f90), wet deposition (wetdepo.f90) and the sparse grid_conc writer with its
// air density (concoutput.f90:176-205, 296-447).
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#include "fpx_step_common.hpp"
#include <cstddef>

namespace fpx {
FPX_TU_OPEN

// ---------------------------------------------------------------------------
// concoutput.f90:296-447 -- the sparse grid_conc writer.  For one (species, pointspec,
// age class): class mean of the sampling grid, the non-zero test, and the run-length compression (start index
// of every run of non-zero cells; values with a sign that flips from run to run) as two scans and two
// element-wise kernels.  Arithmetic in float, the reference's own kind for this routine, contraction off.
// ---------------------------------------------------------------------------
template <typename G>
__global__ void __launch_bounds__(kBlock) k_co_values(const G *__restrict__ grid, size_t class_stride, int nclass, long long n,
                                                      float *__restrict__ val, unsigned int *__restrict__ nz, unsigned int *__restrict__ rs) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  auto value = [&](long long j) -> float {          // mean_mod.f90:mean_sp, times nclassunc (concoutput.f90:323-325)
    float xl = 0.f;
    for (int l = 0; l < nclass; l++) xl = xl + (float)grid[(size_t)l * class_stride + j];
    return (xl / (float)nclass) * (float)nclass;
  };
  const float v = value(i);
  const bool on = v > 1.17549435e-38f;               // smallnum = tiny(0.0)
  const bool prev = i > 0 && value(i - 1) > 1.17549435e-38f;
  val[i] = v;
  nz[i] = on ? 1u : 0u;
  rs[i] = (on && !prev) ? 1u : 0u;                   // sp_zer: a run starts here
}

__global__ void __launch_bounds__(kBlock) k_co_write(const float *__restrict__ val, const unsigned int *__restrict__ nz, const unsigned int *__restrict__ rs,
                                                     const unsigned int *__restrict__ rpos /* exclusive scan of nz */,
                                                     const unsigned int *__restrict__ runid /* inclusive scan of rs */, long long n,
                                                     const float *__restrict__ scale /* volume (conc, pptv) or area, per cell */, int conc, float outnum, float tot_mu,
                                                     int idx0, int *__restrict__ wi, float *__restrict__ wr,
                                                     const float *__restrict__ dens = nullptr, float weightmolar = 1.f) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !nz[i]) return;
  const unsigned int run = runid[i];
  const float sp_fact = (run & 1u) ? 1.f : -1.f;     // sp_fact starts at -1 and flips at every run start
  if (rs[i]) wi[run - 1] = (int)i + idx0;
  float r;
  if (conc == 2) {                                     // mixing ratio, concoutput.f90:575-579
    r = sp_fact * 1.e12f * val[i] / scale[i] / outnum * 28.97f / weightmolar / dens[i];
  } else if (conc) {
    const float f3 = 1.e12f / scale[i] / outnum;     // factor3d, concoutput.f90:226 (ldirect = 1)
    r = sp_fact * val[i] * f3 / tot_mu;
  } else r = sp_fact * 1.e12f * val[i] / scale[i];
  wr[rpos[i]] = r;
}

// densityoutgrid, concoutput.f90:176-205: air density at the centre of every output cell from the met density of slot
// memind(2) (the r2 pack), nearest column, linear between the two z levels around the mid height of the output layer
template <typename R>
__global__ void __launch_bounds__(kBlock) k_co_density(View<R> V, int nxg, int nyg, int nzg, const float *__restrict__ outheight,
                                                       float dxout, float dyout, float outlon0, float outlat0, float dx, float dy, float xlon0, float ylat0,
                                                       float *__restrict__ dens) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)nxg * nyg * nzg) return;
  const int ix = (int)(i % nxg), jy = (int)((i / nxg) % nyg), kz = 1 + (int)(i / ((long long)nxg * nyg));
  const float halfheight = kz == 1 ? outheight[0] / 2.f : (outheight[kz - 1] + outheight[kz - 2]) / 2.f;
  int kzz;
  for (kzz = 2; kzz <= V.nz; kzz++)
    if ((float)V.height[kzz - 2] < halfheight && (float)V.height[kzz - 1] > halfheight) break;
  kzz = max(min(kzz, V.nz), 2);
  const float dz1 = halfheight - (float)V.height[kzz - 2], dz2 = (float)V.height[kzz - 1] - halfheight, dz = dz1 + dz2;
  float xl = outlon0 + (float)ix * dxout, yl = outlat0 + (float)jy * dyout;
  xl = (xl - xlon0) / dx;
  yl = (yl - ylat0) / dy;
  const int iix = max(min((int)lroundf(xl), V.nxmin1), 0), jjy = max(min((int)lroundf(yl), V.nymin1), 0);
  const size_t col = ((size_t)jjy * V.nx + iix) * V.nz;
  const float r1 = (float)V.r2[(col + (kzz - 1)) * 4 + V.m2 * 2], r0 = (float)V.r2[(col + (kzz - 2)) * 4 + V.m2 * 2];
  dens[i] = (r1 * dz1 + r0 * dz2) / dz;
}

// conccalc.f90:50-295: every slot, whole waves stay convergent for the wave-level pre-reduction
template <typename R>
__global__ void __launch_bounds__(kBlock) k_conccalc(View<R> V_arg, GridP<R> Gp_arg, Parts<R> P_arg, long long numpart, int itime, R weight) {
#ifndef FPX_VIEW_BY_VALUE
  struct KArgs { View<R> V; GridP<R> Gp; Parts<R> P; };
  const KArgs &ka = *(const KArgs *)(const void *)__builtin_amdgcn_kernarg_segment_ptr();
  const View<R> &V = ka.V; const GridP<R> &Gp = ka.Gp; const Parts<R> &P = ka.P;
  (void)V_arg; (void)Gp_arg; (void)P_arg;
#else
  const View<R> &V = V_arg; const GridP<R> &Gp = Gp_arg; const Parts<R> &P = P_arg;
#endif
  __shared__ R hgt[kMaxNz];
  __shared__ R outh[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  for (int k = threadIdx.x; k < Gp.numzgrid; k += blockDim.x) outh[k] = Gp.outheight[k];
  __syncthreads();
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool active = s < numpart;
  double xt = 0, yt = 0;
  R zt = 0, xm[kMaxSpec];
  int itage = 0, npoint = 1, nclass = 1;
#pragma unroll
  for (int ks = 0; ks < kMaxSpec; ks++) xm[ks] = (R)0;
  if (active) {
    // the particle's state in ONE memory round trip (nearly every particle is due; the asm keeps the compiler from sinking
    // each load behind the branch that first needs it)
    int itra1 = P.itra1[s], itramem = P.itramem[s];
    xt = P.xt[s]; yt = P.yt[s]; zt = P.zt[s];
    npoint = P.npoint[s]; nclass = P.nclass[s];
#pragma unroll
    for (int ks = 0; ks < kMaxSpec; ks++)
      if (ks < V.nspec) xm[ks] = P.xmass1[(size_t)ks * P.cap + s];
    static_assert(kMaxSpec == 5, "the tie below names five species");
    asm volatile("" : "+v"(itra1), "+v"(itramem), "+v"(xt), "+v"(yt), "+v"(zt), "+v"(npoint), "+v"(nclass),
                      "+v"(xm[0]), "+v"(xm[1]), "+v"(xm[2]), "+v"(xm[3]), "+v"(xm[4]));
    itage = abs(itime - itramem);
    active = itra1 == itime;
    if (!(xt >= 0. && xt <= (double)V.nxmin1 && yt >= 0. && yt <= (double)V.nymin1) || !(zt == zt)) active = false;
  }
  if (P.xscav) {   // wave-uniform: DRYBKDEP / WETBKDEP
    R sc[kMaxSpec];
#pragma unroll
    for (int ks = 0; ks < kMaxSpec; ks++) sc[ks] = (active && ks < V.nspec) ? m_max(P.xscav[(size_t)ks * P.cap + s], (R)0) : (R)0;
    conccalc_particle(V, Gp, hgt, active, xt, yt, zt, itage, npoint, nclass, xm, weight, sc, outh);
  } else {
    conccalc_particle(V, Gp, hgt, active, xt, yt, zt, itage, npoint, nclass, xm, weight, (const R *)nullptr, outh);
  }
}

// The receptor block of timemanager.f90:564-598 (backward runs with DRYBKDEP / WETBKDEP): once per particle, before it is
// moved for the first time -- xscav_frac1 < 0 marks a particle that has not been through it (releaseparticles.f90:167-171).
// get_vdep_prob.f90 sets the cell (the nest's inside a nest) but not the weights p1..p4, dt1, dt2, dtt that
// interpol_vdep[_nests] reads: those are the ones initialize() of the same particle left in interpol_mod, i.e. the
// mother grid's weights at the particle's position and the step's time weights -- computed here from the position.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_bkdep(View<R> V_arg, WetP<R> Wp, Parts<R> P, long long numpart, int itime, int drybkdep, int wetbkdep,
                                                  const R *__restrict__ zspan /* [numpoint] zpoint2 - zpoint1 */) {
  FPX_VIEW_FROM_KERNARG(V, V_arg);
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  __syncthreads();
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart) return;
  if (P.itra1[s] != itime) return;
  bool todo = false;
  for (int ks = 0; ks < V.nspec; ks++) todo = todo || P.xscav[(size_t)ks * P.cap + s] < (R)0;
  if (!todo) return;
  const double xt = P.xt[s], yt = P.yt[s];
  const R zt = P.zt[s];
  if (!(xt >= 0. && xt <= (double)V.nxmin1 && yt >= 0. && yt <= (double)V.nymin1) || !(zt == zt)) return;   // k_prep terminates it
  if (drybkdep) {
    const R href = (R)15.;
    // get_vdep_prob.f90:52-99
    const int ngrid = pick_grid<R, false>(V, xt, yt);
    int ix, jy;
    if (ngrid > 0) {
      const NestDesc<R> &N = V.nest[ngrid - 1];
      ix = (int)(R)((xt - (double)N.xl) * (double)N.xres);
      jy = (int)(R)((yt - (double)N.yl) * (double)N.yres);
    } else {
      ix = (int)xt; jy = (int)yt;
    }
    Cell<R> C;
    cell_setup(C, ix, jy, ix + 1, jy + 1, (R)xt, (R)yt);
    {   // the weights of initialize(): ddx = real(xt) - real(int(xt)) on the mother grid
      const int ixm = (int)xt, jym = (int)yt;
      const R ddx = (R)xt - (R)ixm, ddy = (R)yt - (R)jym, rddx = (R)1 - ddx, rddy = (R)1 - ddy;
      C.p1 = rddx * rddy; C.p2 = ddx * rddy; C.p3 = rddx * ddy; C.p4 = ddx * ddy;
    }
    const Fld<R> F = fld_of(V, ngrid);
    const TimeW<R> W = time_weights(V, itime);
    for (int ks = 0; ks < V.nspec; ks++) {
      if (!(P.xscav[(size_t)ks * P.cap + s] < (R)0)) continue;
      if (V.drydepspec[ks]) {
        R prob = (R)0;
        if (V.drydep && zt < (R)2. * href) prob = interp_vdep(V, F, C, W, ks);   // :105-127: the deposition velocity itself
        P.xscav[(size_t)ks * P.cap + s] = prob;
      } else {
        P.xmass1[(size_t)ks * P.cap + s] = (R)0;
        P.xscav[(size_t)ks * P.cap + s] = (R)0;
      }
    }
  }
  if (wetbkdep) {
    const int np = release_index(V, P.npoint[s]);
    for (int ks = 0; ks < V.nspec; ks++) {
      if (!(P.xscav[(size_t)ks * P.cap + s] < (R)0)) continue;
      R grfr = (R)0;
      const R wetscav = get_wetscav(V, Wp, hgt, itime, V.lsynctime, xt, yt, zt, ks, grfr);
      if (wetscav > (R)0) {
        P.xscav[(size_t)ks * P.cap + s] = wetscav * zspan[np] * grfr;
      } else {
        P.xmass1[(size_t)ks * P.cap + s] = (R)0;
        P.xscav[(size_t)ks * P.cap + s] = (R)0;
      }
    }
  }
}

// wetdepo.f90:58-151: every live particle that is due or overdue
template <typename R>
__global__ void __launch_bounds__(kBlock) k_wetdepo(View<R> V_arg, GridP<R> Gp_arg, WetP<R> Wp_arg, Parts<R> P_arg, long long numpart, int itime,
                                                    int ltsample, int loutnext) {
#ifndef FPX_VIEW_BY_VALUE
  struct KArgs { View<R> V; GridP<R> Gp; WetP<R> Wp; Parts<R> P; };
  const KArgs &ka = *(const KArgs *)(const void *)__builtin_amdgcn_kernarg_segment_ptr();
  const View<R> &V = ka.V; const GridP<R> &Gp = ka.Gp; const WetP<R> &Wp = ka.Wp; const Parts<R> &P = ka.P;
  (void)V_arg; (void)Gp_arg; (void)Wp_arg; (void)P_arg;
#else
  const View<R> &V = V_arg; const GridP<R> &Gp = Gp_arg; const WetP<R> &Wp = Wp_arg; const Parts<R> &P = P_arg;
#endif
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  __syncthreads();
  // every lane stays to the end (the wave-level sums of wetdepo_scatter need convergent waves): `live` says whether the lane
  // holds a particle that is scavenged at all
  const long long s0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool live = s0 < numpart;
  const long long s = live ? s0 : 0;
  // the particle's state in ONE memory round trip (as in k_conccalc)
  int itra1 = P.itra1[s], itramem = P.itramem[s], nunc = P.nclass[s];
  int kp = Gp.ioutputforeachrelease == 1 ? P.npoint[s] : 1;
  double xt = P.xt[s], yt = P.yt[s];
  R zt = P.zt[s];
  R xm_all[kMaxSpec];
#pragma unroll
  for (int ks = 0; ks < kMaxSpec; ks++) xm_all[ks] = (ks < V.nspec && Wp.wetdepspec[ks]) ? P.xmass1[(size_t)ks * P.cap + s] : (R)0;
  static_assert(kMaxSpec == 5, "the tie below names five species");
  asm volatile("" : "+v"(itra1), "+v"(itramem), "+v"(nunc), "+v"(kp), "+v"(xt), "+v"(yt), "+v"(zt),
                    "+v"(xm_all[0]), "+v"(xm_all[1]), "+v"(xm_all[2]), "+v"(xm_all[3]), "+v"(xm_all[4]));
  if (itra1 == kDead) live = false;
  if (V.ldirect == 1) { if (itra1 > itime) live = false; } else { if (itra1 < itime) live = false; }
  if (!(xt >= 0. && xt <= (double)V.nxmin1 && yt >= 0. && yt <= (double)V.nymin1) || !(zt == zt)) live = false;
  if (!live) { xt = 0.; yt = 0.; zt = (R)0; }      // a harmless position for the lanes that only take part in the sums
  const int ldeltat = itime <= loutnext ? itime - (loutnext - Gp.loutstep) : itime - loutnext;   // wetdepo.f90:58-62
  const int nage = ageclass(Gp, abs(itra1 - itramem));
  const R smallnum = sizeof(R) == 4 ? (R)1.17549435e-38f : (R)2.2250738585072014e-308;
  for (int ks = 0; ks < V.nspec; ks++) {
    if (!Wp.wetdepspec[ks]) continue;
    R grfr = (R)0;
    R wetdeposit = (R)0;
    if (live) {
      const R wetscav = get_wetscav(V, Wp, hgt, itime, ltsample, xt, yt, zt, ks, grfr);
      const R xm = pick(xm_all, ks);
      if (wetscav > (R)0) wetdeposit = xm * ((R)1 - m_exp(-wetscav * (R)abs(ltsample))) * grfr;
      const R restmass = xm - wetdeposit;
      P.xmass1[(size_t)ks * P.cap + s] = restmass > smallnum ? restmass : (R)0;
      if (V.decay[ks] > (R)0) wetdeposit = wetdeposit * m_exp((R)abs(ldeltat) * V.decay[ks]);
    }
    if (V.ldirect == 1 && Gp.on) wetdepo_scatter(V, Gp, nunc, wetdeposit, ks, (R)xt, (R)yt, nage, kp);
    if (V.ldirect == 1 && Gp.on && Gp.nested) wetdepo_scatter(V, Gp, nunc, wetdeposit, ks, (R)xt, (R)yt, nage, kp, true);   // wetdepo.f90:142
  }
}

FPX_TU_CLOSE
}  // namespace fpx
