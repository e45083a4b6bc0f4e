// Device side of the gross mass fluxes: calcfluxes.f90:43-166, which the particle loop calls after advance
// (timemanager.f90:623) when iflux = 1, run by fpx_step when fpx_config.device_flux is set.
//
// Two kernels around the three of the step, a lane per storage space.  k_flux_save (after the receptor block k_bkdep,
// before k_prep) keeps what calcfluxes needs from before the move: xold, yold, zold of timemanager.f90:560-562 -- default
// reals there, so the positions are stored converted to the host's real kind H -- and xmass1 as the epilogue has not yet
// touched it, and marks the space due.  k_calcfluxes (after k_pbl_finish) reads them back together with the new position,
// npoint and itramem, all coalesced streams, and adds the particle's masses to the faces it crossed.
// The types are the reference's declarations: xtra1, ytra1 double, everything else in H; an expression that mixes the two is
// formed in double.  FMA contraction is off and the divisions are IEEE, no libm is involved, so every cell decision is the
// reference's, bit for bit.  flux has the reference's element order (outgrid_init.f90:186):
// (6, 0:numxgrid-1, 0:numygrid-1, numzgrid, nspec, maxpointspec_act, nageclass), first index fastest.
// The per-particle body compiles as host code too (FPX_CF_HOST: a plain += for the atomic), for checks without a GPU.
#pragma once
#ifndef FPX_CF_HOST
#include "fpx_tu.hpp"
#include <hip/hip_runtime.h>
#define FPX_CF_FN __device__ __forceinline__
#else
#include <cstddef>
#define FPX_CF_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif

namespace fpx {
FPX_TU_OPEN
namespace cf {

constexpr int kMaxAgeCf = 8;        // FPX_MAXAGECLASS

template <typename H>
struct Args {
  int numxgrid, numygrid, numzgrid, nspec, maxpointspec_act, nageclass;
  int use_npoint;                    // ioutputforeachrelease == 1 && mdomainfill == 0 (calcfluxes.f90:43)
  int nx, nxmin1;
  int lage[kMaxAgeCf];
  H dx, dy, dxout, dyout, xoutshift, youtshift;
  const H *outheight, *outheighthalf;    // [numzgrid]
  H *flux;
  // what k_flux_save keeps of the state before the move
  H *xold, *yold, *zold;             // [cap]
  H *mass;                           // [nspec][cap]
  unsigned char *due;                // [cap]
  long long cap;
};

#ifndef FPX_CF_HOST
template <typename H> FPX_CF_FN void cf_add(H *p, H v) { atomicAdd(p, v); }
#else
template <typename H> FPX_CF_FN void cf_add(H *p, H v) { *p += v; }
#endif

// Fortran's int(): truncation toward zero.  Values beyond the integer range (no sane grid has them) saturate instead of
// leaving the conversion undefined; every use is range-tested afterwards.
template <typename T>
FPX_CF_FN int cf_int(T v) {
  if (v >= (T)2147483520.) return 2147483647;
  if (v <= (T)-2147483520.) return -2147483647;
  return (int)v;
}
FPX_CF_FN int cf_min(int a, int b) { return a < b ? a : b; }
FPX_CF_FN int cf_max(int a, int b) { return a > b ? a : b; }

// calcfluxes.f90:43-166 for one particle.  mass[k * mstride]: xmass1(jpart,k) as it was before the epilogue.
// Guards without a counterpart in the reference: nage beyond nageclass and kp outside 1..maxpointspec_act contribute nothing
// (the reference would write outside flux); the caller has tested the new position for finiteness.
template <typename H>
FPX_CF_FN void flux_particle(const Args<H> &A, H xold, H yold, H zold, double xtra1, double ytra1, H ztra1, int npoint, int itage,
                             const H *mass, size_t mstride) {
#pragma clang fp contract(off)
  int nage = 1;                                            // timemanager.f90:545-548
  for (; nage <= A.nageclass; nage++)
    if (itage < A.lage[nage - 1]) break;
  const int kp = A.use_npoint ? npoint : 1;
  if (nage > A.nageclass || kp < 1 || kp > A.maxpointspec_act) return;
  const int nxg = A.numxgrid, nyg = A.numygrid, nzg = A.numzgrid;
  // element (1, 0, 0, 1, 1, kp, nage); the species stride
  const size_t sstride = (size_t)6 * nxg * nyg * nzg;
  H *const f0 = A.flux + sstride * (size_t)A.nspec * ((size_t)(kp - 1) + (size_t)A.maxpointspec_act * (size_t)(nage - 1));
  auto cell = [&](int i, int ix, int jy, int kz) -> size_t { return (size_t)(i - 1) + 6 * ((size_t)ix + (size_t)nxg * ((size_t)jy + (size_t)nyg * (size_t)(kz - 1))); };

  const H xmean = (H)(((double)xold + xtra1) / 2.);
  const H ymean = (H)(((double)yold + ytra1) / 2.);
  const int ixave = cf_int((xmean * A.dx + A.xoutshift) / A.dxout);
  const int jyave = cf_int((ymean * A.dy + A.youtshift) / A.dyout);
  int kz;
  for (kz = 1; kz <= nzg; kz++)
    if (A.outheight[kz - 1] > ztra1) break;
  const int kzave = kz;

  // vertical fluxes, :63-86
  if (ixave >= 0 && jyave >= 0 && ixave <= nxg - 1 && jyave <= nyg - 1) {
    for (kz = 1; kz <= nzg; kz++)
      if (A.outheighthalf[kz - 1] > zold) break;
    const int k1 = cf_min(nzg, kz);
    for (kz = 1; kz <= nzg; kz++)
      if (A.outheighthalf[kz - 1] > ztra1) break;
    const int k2 = cf_min(nzg, kz);
    for (int k = 0; k < A.nspec; k++) {
      const H m = mass[(size_t)k * mstride];
      for (kz = k1; kz <= k2 - 1; kz++) cf_add(f0 + sstride * k + cell(5, ixave, jyave, kz), m);
      for (kz = k2; kz <= k1 - 1; kz++) cf_add(f0 + sstride * k + cell(6, ixave, jyave, kz), m);
    }
  }

  // west-east and east-west fluxes, :92-139
  if (kzave <= nzg && jyave >= 0 && jyave <= nyg - 1) {
    double d = (double)xold - xtra1;
    if (d < 0.) d = -d;
    if (d < (double)((H)A.nx / (H)2.)) {
      const int ix1 = cf_int((xold * A.dx + A.xoutshift) / A.dxout + (H)0.5);
      const int ix2 = cf_int((xtra1 * (double)A.dx + (double)A.xoutshift) / (double)A.dxout + 0.5);
      // do ix=ix1,ix2-1 / do ix=ix2,ix1-1 with their range tests: the loops clipped to the grid
      const int a1 = cf_max(ix1, 0), b1 = cf_min(ix2 - 1, nxg - 1), a2 = cf_max(ix2, 0), b2 = cf_min(ix1 - 1, nxg - 1);
      for (int k = 0; k < A.nspec; k++) {
        const H m = mass[(size_t)k * mstride];
        for (int ix = a1; ix <= b1; ix++) cf_add(f0 + sstride * k + cell(1, ix, jyave, kzave), m);
        for (int ix = a2; ix <= b2; ix++) cf_add(f0 + sstride * k + cell(2, ix, jyave, kzave), m);
      }
    } else {
      // the cyclic branch exactly as written (:122): for any sane grid ixs is negative and nothing is added
      const int ixs = cf_int((((H)A.nxmin1 - (H)1.e5) * A.dx + A.xoutshift) / A.dxout);
      if (ixs >= 0 && ixs <= nxg - 1) {
        const int i = (double)xold > xtra1 ? 1 : 2;
        for (int k = 0; k < A.nspec; k++) cf_add(f0 + sstride * k + cell(i, ixs, jyave, kzave), mass[(size_t)k * mstride]);
      }
    }
  }

  // south-north and north-south fluxes, :145-166
  if (kzave <= nzg && ixave >= 0 && ixave <= nxg - 1) {
    const int jy1 = cf_int((yold * A.dy + A.youtshift) / A.dyout + (H)0.5);
    const int jy2 = cf_int((ytra1 * (double)A.dy + (double)A.youtshift) / (double)A.dyout + 0.5);
    const int a1 = cf_max(jy1, 0), b1 = cf_min(jy2 - 1, nyg - 1), a2 = cf_max(jy2, 0), b2 = cf_min(jy1 - 1, nyg - 1);
    for (int k = 0; k < A.nspec; k++) {
      const H m = mass[(size_t)k * mstride];
      for (int jy = a1; jy <= b1; jy++) cf_add(f0 + sstride * k + cell(3, ixave, jy, kzave), m);
      for (int jy = a2; jy <= b2; jy++) cf_add(f0 + sstride * k + cell(4, ixave, jy, kzave), m);
    }
  }
}

#ifndef FPX_CF_HOST
// timemanager.f90:537,560-562: every space that is due keeps its position and masses; the others are marked not due
template <typename H, typename R>
__global__ void __launch_bounds__(256) k_flux_save(Args<H> A, const double *__restrict__ xt, const double *__restrict__ yt, const R *__restrict__ zt,
                                                   const R *__restrict__ xmass1, const int *__restrict__ itra1, long long pcap, long long numpart, int itime) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart) return;
  const bool due = itra1[s] == itime;
  A.due[s] = due ? 1 : 0;
  if (!due) return;
  A.xold[s] = (H)xt[s];
  A.yold[s] = (H)yt[s];
  A.zold[s] = (H)zt[s];
  for (int k = 0; k < A.nspec; k++) A.mass[(size_t)k * A.cap + s] = (H)xmass1[(size_t)k * pcap + s];
}

template <typename H, typename R>
__global__ void __launch_bounds__(256) k_calcfluxes(Args<H> A, const double *__restrict__ xt, const double *__restrict__ yt, const R *__restrict__ zt,
                                                    const int *__restrict__ npoint, const int *__restrict__ itramem, long long numpart, int itime) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart) return;
  if (!A.due[s]) return;
  const double xtra1 = xt[s], ytra1 = yt[s];
  const H ztra1 = (H)zt[s];
  if (!(xtra1 - xtra1 == 0.) || !(ytra1 - ytra1 == 0.) || !(ztra1 - ztra1 == (H)0)) return;   // not finite: no flux
  const int itage = abs(itime - itramem[s]);
  flux_particle<H>(A, A.xold[s], A.yold[s], A.zold[s], xtra1, ytra1, ztra1, npoint[s], itage, A.mass + s, (size_t)A.cap);
}
#endif

}  // namespace cf
FPX_TU_CLOSE
}  // namespace fpx
