// Device side of the potential vorticity on model levels: calcpv.f90:42-313 for the mother grid and calcpv_nests.f90 (the
// same algorithm with the nest's geometry and no global flags) for a nest, run by fpx_verttransform_ecmwf / _nest when
// fpx_model_levels.pvh is NULL.  Everything it reads (uuh, vvh, tth, ps, akz, bkz) is already on the device, in the host's
// layout, when the transform starts; it writes pvh where the transform reads it.
//
// Two steps.  k_theta: ppml = akz + bkz*ps, ppmk = (100000./ppml)**kappa, theta = tth*ppmk, one pow per grid point; ppml and
// theta are stored (the reference recomputes tth*ppmk at every use: the product of the same two numbers is the same number).
// k_pv: per point dthetadp, the spiral search for the theta surface in the two x- and the two y-neighbours (up first, then
// down, the goto order of calcpv.f90:133-190, :209-263), vx, uy, jux/juy, the same-level fallback, pvh.  k_pole: the mean of
// the neighbouring ring per level, summed serially in ix as the reference does (:288-313).
// One lane per grid point, the level in blockIdx.y: consecutive lanes own consecutive ix of the flattened (ix,jy) index, so a
// wave reads one row segment (two where it crosses a row end) of every array it touches.
// Arithmetic in the host's real kind H with FMA contraction off; pow, sin, cos, tan come from the device's libm.
#pragma once
#include "fpx_tu.hpp"
#include <hip/hip_runtime.h>
#include "fpx_verttransform.hpp"

namespace fpx {
FPX_TU_OPEN
namespace pv {

#ifndef CK
#define CK(x) ((H)(x))
#endif

template <typename H> __device__ __forceinline__ H m_tan(H x);
template <> __device__ __forceinline__ float m_tan<float>(float x) { return ::tanf(x); }
template <> __device__ __forceinline__ double m_tan<double>(double x) { return ::tan(x); }

template <typename H>
struct Args {
  int nx, ny, nuvz, nxmax, nymax;    // extents and the strides of the host's arrays
  int xglobal, nglobal, sglobal;     // all 0 on a nest
  H dx, dy, ylat0;                   // dx, dy, ylat0 (mother) or dxn(l), dyn(l), ylat0n(l)
  const H *uuh, *vvh, *tth;          // (0:nxmax-1,0:nymax-1,nuvz)
  const H *ps;                       // (0:nxmax-1,0:nymax-1)
  const H *akz, *bkz;                // (nuvz)
  H *ppml, *theta;                   // scratch, (0:nxmax-1,0:nymax-1,nuvz)
  H *pvh;                            // out
};

// calcpv.f90:46-55 and the product of :106
template <typename H>
__global__ void __launch_bounds__(256) k_theta(Args<H> A) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.nx * A.ny) return;
  const int ix = c % A.nx, jy = c / A.nx, kl = blockIdx.y;       // kl 0-based here
  const size_t i2 = (size_t)ix + (size_t)A.nxmax * (size_t)jy;
  const size_t i3 = i2 + (size_t)A.nxmax * (size_t)A.nymax * (size_t)kl;
  const H p = A.akz[kl] + A.bkz[kl] * A.ps[i2];
  const H pk = vt::M<H>::pow(CK(100000.) / p, CK(0.286));        // kappa, par_mod.f90:60
  A.ppml[i3] = p;
  A.theta[i3] = A.tth[i3] * pk;
}

// One neighbour column of the spiral search (calcpv.f90:133-190 / :209-263): th, w address level 1 of the neighbour's
// column, `plane` is the level stride; kl, k are 1-based as in the reference.  Returns false when no bracket was found
// within nlck tests (label 21 / 51).
template <typename H>
__device__ __forceinline__ bool spiral(const H *th, const H *w, size_t plane, H theta, int kl, int nuvz, int nlck, H &val) {
#pragma clang fp contract(off)
  const H eps = CK(1.e-5);
  int kup = kl - 1, kdn = kl, kch = 0;
  for (;;) {
    kup = kup + 1;                                               // 40: upward branch
    if (kch >= nlck) return false;
    int k = 0;
    if (kup < nuvz) {
      kch = kch + 1;
      k = kup;
    } else {
      kdn = kdn - 1;                                             // 41: downward branch
      if (kdn < 1) continue;
      kch = kch + 1;
      k = kdn;
    }
    for (;;) {
      const H thdn = th[plane * (size_t)(k - 1)], thup = th[plane * (size_t)k];
      if ((thdn >= theta && thup <= theta) || (thdn <= theta && thup >= theta)) {
        H dt1 = fabs(theta - thdn), dt2 = fabs(theta - thup), dt = dt1 + dt2;
        if (dt < eps) { dt1 = CK(0.5); dt2 = CK(0.5); dt = CK(1.0); }
        val = (w[plane * (size_t)(k - 1)] * dt2 + w[plane * (size_t)k] * dt1) / dt;
        return true;
      }
      if (k != kup) break;                                       // that was the downward test: back to 40
      kdn = kdn - 1;                                             // after a failed upward test: 41
      if (kdn < 1) break;
      kch = kch + 1;
      k = kdn;
    }
  }
}

template <typename H>
__global__ void __launch_bounds__(256) k_pv(Args<H> A) {
#pragma clang fp contract(off)
  typedef vt::M<H> M;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.nx * A.ny) return;
  const int nx = A.nx, ny = A.ny, nuvz = A.nuvz;
  const int ix = c % nx, jy = c / nx, kl = (int)blockIdx.y + 1;
  if (A.sglobal && jy == 0) return;                              // the pole rows are k_pole's
  if (A.nglobal && jy == ny - 1) return;
  const int nlck = nuvz / 3;
  const size_t sx = (size_t)A.nxmax, plane = (size_t)A.nxmax * (size_t)A.nymax;
  const size_t i2 = (size_t)ix + sx * (size_t)jy, i3 = i2 + plane * (size_t)(kl - 1);
  const H pi = CK(3.14159265), r_earth = CK(6.371e6);            // par_mod.f90:59
  const H phi = (A.ylat0 + CK(jy) * A.dy) * pi / CK(180.);
  const H f = CK(0.00014585) * M::sin(phi);
  const H tanphi = m_tan<H>(phi), cosphi = M::cos(phi);
  // virtual neighbours at the domain edge (:64-100)
  int jyvp = jy + 1, jyvm = jy - 1;
  if (jy == 0) jyvm = 0;
  if (jy == ny - 1) jyvp = ny - 1;
  int jumpy = 2;
  if (jy == 0 || jy == ny - 1) jumpy = 1;
  if (A.sglobal && jy == 1) { jyvm = 1; jumpy = 1; }
  if (A.nglobal && jy == ny - 2) { jyvp = ny - 2; jumpy = 1; }
  int ixvp = ix + 1, ixvm = ix - 1, jumpx = 2, ivrp, ivrm;
  if (A.xglobal) {
    ivrp = ixvp; ivrm = ixvm;
    if (ixvm < 0) ivrm = ixvm + (nx - 1);                        // the grid carries the duplicated meridian
    if (ixvp >= nx) ivrp = ixvp - nx + 1;
  } else {
    if (ix == 0) ixvm = 0;
    if (ix == nx - 1) ixvp = nx - 1;
    ivrp = ixvp; ivrm = ixvm;
    if (ix == 0 || ix == nx - 1) jumpx = 1;
  }
  const H theta = A.theta[i3];
  int klvrp = kl + 1, klvrm = kl - 1;
  if (klvrp > nuvz) klvrp = nuvz;
  if (klvrm < 1) klvrm = 1;
  const size_t ip = i2 + plane * (size_t)(klvrp - 1), im = i2 + plane * (size_t)(klvrm - 1);
  const H dthetadp = (A.theta[ip] - A.theta[im]) / (A.ppml[ip] - A.ppml[im]);
  // a) in x direction: i = ixvm, ixvp (do i=ixvm,ixvp,jumpx always has these two members)
  int jux = jumpx;
  H vx[2];
#pragma unroll
  for (int ii = 0; ii < 2; ii++) {
    const int ivr = ii == 0 ? ivrm : ivrp;
    const size_t col = (size_t)ivr + sx * (size_t)jy;
    if (!spiral<H>(A.theta + col, A.vvh + col, plane, theta, kl, nuvz, nlck, vx[ii])) {
      vx[ii] = A.vvh[i3];
      jux = jux - 1;
    }
  }
  H dvdx;
  if (jux > 0) dvdx = (vx[1] - vx[0]) / CK(jux) / (A.dx * pi / CK(180.));
  else {
    dvdx = A.vvh[(size_t)ivrp + sx * (size_t)jy + plane * (size_t)(kl - 1)] - A.vvh[(size_t)ivrm + sx * (size_t)jy + plane * (size_t)(kl - 1)];
    dvdx = dvdx / CK(jumpx) / (A.dx * pi / CK(180.));
  }
  // b) in y direction: j = jyvm, jyvp
  int juy = jumpy;
  H uy[2];
#pragma unroll
  for (int jj = 0; jj < 2; jj++) {
    const int j = jj == 0 ? jyvm : jyvp;
    const size_t col = (size_t)ix + sx * (size_t)j;
    if (!spiral<H>(A.theta + col, A.uuh + col, plane, theta, kl, nuvz, nlck, uy[jj])) {
      uy[jj] = A.uuh[i3];
      juy = juy - 1;
    }
  }
  H dudy;
  if (juy > 0) dudy = (uy[1] - uy[0]) / CK(juy) / (A.dy * pi / CK(180.));
  else {
    dudy = A.uuh[(size_t)ix + sx * (size_t)jyvp + plane * (size_t)(kl - 1)] - A.uuh[(size_t)ix + sx * (size_t)jyvm + plane * (size_t)(kl - 1)];
    dudy = dudy / CK(jumpy) / (A.dy * pi / CK(180.));
  }
  A.pvh[i3] = dthetadp * (f + (dvdx / cosphi - dudy + A.uuh[i3] * tanphi) / r_earth) * CK(-1.e6) * CK(9.81);
}

// calcpv.f90:288-313: blockIdx.y = 0 the south pole row (from row 1), 1 the north pole row (from row ny-2); one lane per
// level sums the ring in the reference's order ix = 0..nx-1 and fills the pole row
template <typename H>
__global__ void __launch_bounds__(64) k_pole(Args<H> A) {
#pragma clang fp contract(off)
  const int kl = blockIdx.x * blockDim.x + threadIdx.x;
  if (kl >= A.nuvz) return;
  const bool north = blockIdx.y == 1;
  if (north ? !A.nglobal : !A.sglobal) return;
  const size_t sx = (size_t)A.nxmax, plane = (size_t)A.nxmax * (size_t)A.nymax;
  H *ring = A.pvh + plane * (size_t)kl + sx * (size_t)(north ? A.ny - 2 : 1);
  H *pole = A.pvh + plane * (size_t)kl + sx * (size_t)(north ? A.ny - 1 : 0);
  H pvavr = CK(0.);
  for (int ix = 0; ix < A.nx; ix++) pvavr = pvavr + ring[ix];
  pvavr = pvavr / CK(A.nx);
  for (int ix = 0; ix < A.nx; ix++) pole[ix] = pvavr;
}

}  // namespace pv
FPX_TU_CLOSE
}  // namespace fpx
