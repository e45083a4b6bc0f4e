// Device side of the sensitivity to initial conditions of a backward run: initial_cond_calc.f90:37-197, which the
// particle loop calls for a particle it terminates (timemanager.f90:631: left the domain; :702: too old) and once at the
// end of the run for every particle still alive (:735-737), run by fpx_step / fpx_initcond_finish when
// fpx_config.device_initcond is set.
//
// The per-particle body (ic_locate, ic_value) finds the cells and the terms; two kernels add them.  k_initcond runs behind
// k_pbl_finish, a lane per storage space: of the spaces k_prep found due (its keys outlive the step) the few the epilogue
// has terminated are told apart from what the step left in memory (see k_initcond) and add their terms with plain atomics.
// k_initcond_finish touches every live particle once per run: its waves stay convergent and the lanes of a wave that
// share a cell are summed into its 3 x 3 neighbourhood before the atomics (wave_kernel_add, as k_conccalc does).
// The types are the reference's declarations: xtra1, ytra1 double, everything else in the host's real kind H; an expression
// that mixes the two is formed in double and rounded on assignment.  FMA contraction is off and the divisions are IEEE, no
// libm is involved, so every cell decision and every term is the reference's, bit for bit; only the order of the sums
// differs.  init_cond has the reference's element order (outgrid_init.f90:296):
// (0:numxgrid-1, 0:numygrid-1, numzgrid, nspec, maxpointspec_act), first index fastest.
// Guards without a counterpart in the reference, each contributes nothing: nrelpointer outside 1..maxpointspec_act (the
// reference would write outside init_cond); a position that is not finite; for linit_cond = 1 a horizontal position
// outside [0, nx-1) x [0, ny-1] (the reference reads rho out of bounds) and a height at or above height(nz) (the reference
// leaves indz undefined).  For linit_cond = 2 a particle outside the met grid follows the reference: its own index tests
// decide.
// The body compiles as host code too (FPX_IC_HOST: a plain += for the atomic), for checks without a GPU.
#pragma once
#ifndef FPX_IC_HOST
#include "fpx_tu.hpp"
#include <hip/hip_runtime.h>
#define FPX_IC_FN __device__ __forceinline__
#else
#include <cstddef>
#define FPX_IC_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif

namespace fpx {
FPX_TU_OPEN
namespace ic {

template <typename H>
struct Args {
  int linit_cond;                    // 1: mass unit (divide by rho at the particle), 2: mass mixing ratio unit
  int nx, ny, nz;                    // met grid
  int numxgrid, numygrid, numzgrid, nspec, maxpointspec_act;
  int use_npoint;                    // ioutputforeachrelease == 1 && mdomainfill == 0 (initial_cond_calc.f90:99-103)
  H dx, dy, dxout, dyout, xoutshift, youtshift;
  const H *outheight;                // [numzgrid]
  H *init_cond;
};

// the cells of one call and their weights: q = 0: (ix, jy), 1: (ix + dix, jy), 2: (ix, jy + djy), 3: (ix + dix, jy + djy)
template <typename H>
struct Hit {
  int ix, jy, dix, djy, kz, kp;
  int direct;                        // :123-133: the whole term goes to (ix, jy)
  int on[4];                         // the cell lies inside the grid
  H w[4];                            // :161,169,180,188
  H rhoi;
};

// Fortran's int(): truncation toward zero.  Values beyond the integer range (no sane grid has them) saturate instead of
// leaving the conversion undefined; every use is range-tested afterwards.
template <typename T>
FPX_IC_FN int ic_int(T v) {
  if (v >= (T)2147483520.) return 2147483647;
  if (v <= (T)-2147483520.) return -2147483647;
  return (int)v;
}

// initial_cond_calc.f90:44-194 without the sums: false = the call adds nothing.  height: [nz]; outheight: [numzgrid] (the
// caller's copy of A.outheight, or A.outheight itself); rho(ix, jy, ind): the air density of the second wind field in memory
// (memind(2)) at level ind = 1..nz, in H.
template <typename H, typename HT, typename Rho>
FPX_IC_FN bool ic_locate(const Args<H> &A, const HT *height, const H *outheight, Rho rho, double xtra1, double ytra1, H ztra1, int npoint, Hit<H> &h) {
#pragma clang fp contract(off)
  if (!(xtra1 - xtra1 == 0.) || !(ytra1 - ytra1 == 0.) || !(ztra1 - ztra1 == (H)0)) return false;   // guard: not finite
  H rhoi = (H)1.;                                                                                     // :84
  if (A.linit_cond == 1) {                                                                            // :46-82
    if (!(xtra1 >= 0.) || !(xtra1 < (double)(A.nx - 1)) || !(ytra1 >= 0.) || !(ytra1 <= (double)(A.ny - 1))) return false;   // guard
    if (!(ztra1 < (H)height[A.nz - 1])) return false;                                                 // guard
    const int ix = (int)xtra1, jy = (int)ytra1;
    const int ixp = ix + 1, jyp = jy + 1;
    const H ddx = (H)(xtra1 - (double)(H)ix), ddy = (H)(ytra1 - (double)(H)jy);
    const H rddx = (H)1. - ddx, rddy = (H)1. - ddy;
    const H p1 = rddx * rddy, p2 = ddx * rddy, p3 = rddx * ddy, p4 = ddx * ddy;
    // do il=2,nz; if (height(il).gt.ztra1(i)) ... (:59-65): the heights increase strictly and the guard above says that
    // height(nz) qualifies, so bisection finds the first il the linear scan finds
    int lo = 2, hi = A.nz;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((H)height[mid - 1] > ztra1) hi = mid; else lo = mid + 1;
    }
    const int indz = lo - 1, indzp = lo;
    const H dz1 = ztra1 - (H)height[indz - 1], dz2 = (H)height[indzp - 1] - ztra1;
    const H dz = (H)1. / (dz1 + dz2);
    H rhoprof[2];
    for (int l = 0; l < 2; l++) {
      const int ind = indz + l;
      // (jyp = ny only for ytra1 = ny - 1, where its weights are zero: the row of the host's padding reads as 0)
      const H r3 = jyp < A.ny ? rho(ix, jyp, ind) : (H)0, r4 = jyp < A.ny ? rho(ixp, jyp, ind) : (H)0;
      rhoprof[l] = p1 * rho(ix, jy, ind) + p2 * rho(ixp, jy, ind) + p3 * r3 + p4 * r4;
    }
    rhoi = (dz1 * rhoprof[1] + dz2 * rhoprof[0]) * dz;
  }
  h.rhoi = rhoi;
  h.kp = A.use_npoint ? npoint : 1;                                                                   // :99-103
  if (h.kp < 1 || h.kp > A.maxpointspec_act) return false;                                            // guard
  int kz;
  for (kz = 1; kz <= A.numzgrid; kz++)                                                                // :105-109
    if (outheight[kz - 1] > ztra1) break;
  if (kz > A.numzgrid) return false;
  h.kz = kz;
  const H xl = (H)((xtra1 * (double)A.dx + (double)A.xoutshift) / (double)A.dxout);                    // :112-117
  const H yl = (H)((ytra1 * (double)A.dy + (double)A.youtshift) / (double)A.dyout);
  int ix = ic_int(xl);
  if (xl < (H)0.) ix = ix - 1;
  int jy = ic_int(yl);
  if (yl < (H)0.) jy = jy - 1;
  h.ix = ix; h.jy = jy;
  const int nxg = A.numxgrid, nyg = A.numygrid;
  const bool okx = ix >= 0 && ix <= nxg - 1, oky = jy >= 0 && jy <= nyg - 1;
  h.direct = (xl < (H)0.5) || (yl < (H)0.5) || (xl > (H)(nxg - 1) - (H)0.5) || (yl > (H)(nyg - 1) - (H)0.5);   // :123-125
  if (h.direct) {
    h.dix = 1; h.djy = 1;
    h.on[0] = okx && oky; h.on[1] = h.on[2] = h.on[3] = 0;
    h.w[0] = (H)1.; h.w[1] = h.w[2] = h.w[3] = (H)0.;
    return h.on[0] != 0;
  }
  const H ddx = xl - (H)ix, ddy = yl - (H)jy;                                                         // :137-153
  H wx, wy;
  if (ddx > (H)0.5) { h.dix = 1; wx = (H)1.5 - ddx; } else { h.dix = -1; wx = (H)0.5 + ddx; }
  if (ddy > (H)0.5) { h.djy = 1; wy = (H)1.5 - ddy; } else { h.djy = -1; wy = (H)0.5 + ddy; }
  const int ixp = ix + h.dix, jyp = jy + h.djy;
  const bool okxp = ixp >= 0 && ixp <= nxg - 1, okyp = jyp >= 0 && jyp <= nyg - 1;
  h.on[0] = okx && oky; h.on[1] = okxp && oky; h.on[2] = okx && okyp; h.on[3] = okxp && okyp;          // :159-194
  h.w[0] = wx * wy;
  h.w[1] = ((H)1. - wx) * wy;
  h.w[2] = wx * ((H)1. - wy);
  h.w[3] = ((H)1. - wx) * ((H)1. - wy);
  return h.on[0] || h.on[1] || h.on[2] || h.on[3];
}

// the term cell q receives from a mass: xmass1(i,ks)/rhoi (:131) or xmass1(i,ks)/rhoi*w (:164,172,183,191)
template <typename H>
FPX_IC_FN H ic_value(const Hit<H> &h, H m, int q) {
#pragma clang fp contract(off)
  return h.direct ? m / h.rhoi : m / h.rhoi * h.w[q];
}

// element (ix, jy, kz, ks = 1, kp) of init_cond; the species stride is numxgrid * numygrid * numzgrid
template <typename H>
FPX_IC_FN long long ic_cell(const Args<H> &A, const Hit<H> &h) {
  const long long plane = (long long)A.numxgrid * A.numygrid;
  return (long long)h.ix + (long long)A.numxgrid * h.jy + plane * (h.kz - 1) + plane * A.numzgrid * (long long)A.nspec * (h.kp - 1);
}

#ifndef FPX_IC_HOST
template <typename H> FPX_IC_FN void ic_add(H *p, H v) { atomicAdd(p, v); }
#else
template <typename H> FPX_IC_FN void ic_add(H *p, H v) { *p += v; }
#endif

// one call of initial_cond_calc for a particle that passed its `itra1(i).ne.itime` test.  mass[k * mstride]: xmass1(i,k).
template <typename H, typename HT, typename Rho, typename M>
FPX_IC_FN void ic_particle(const Args<H> &A, const HT *height, Rho rho, double xtra1, double ytra1, H ztra1, int npoint,
                           const M *mass, size_t mstride) {
  Hit<H> h;
  if (!ic_locate<H>(A, height, A.outheight, rho, xtra1, ytra1, ztra1, npoint, h)) return;
  const long long c0 = ic_cell(A, h), sstride = (long long)A.numxgrid * A.numygrid * A.numzgrid;
  const long long off[4] = {0, h.dix, (long long)h.djy * A.numxgrid, (long long)h.djy * A.numxgrid + h.dix};
  for (int q = 0; q < 4; q++) {
    if (!h.on[q]) continue;
    for (int k = 0; k < A.nspec; k++) ic_add(A.init_cond + c0 + off[q] + sstride * k, ic_value(h, (H)mass[(size_t)k * mstride], q));
  }
}

#ifndef FPX_IC_HOST
// rho of the gather pack (compact nx, ny; [jy][ix][iz][slot][rho, drhodz]) in the second time slot
template <typename R, typename H>
struct PackRho {
  const R *r2;
  int nx, nz, slot;
  __device__ __forceinline__ H operator()(int ix, int jy, int ind) const {
    return (H)r2[(((size_t)jy * nx + ix) * nz + (ind - 1)) * 4 + slot * 2];
  }
};

// timemanager.f90:630-632 and :701-703 behind the step's epilogue.  A space that was due (key) and is terminated now is
// one of three, and what the step left in memory tells which:
//   position outside the grid (the test of advance's boundary block, which set nstop = 3)  -> :631, contributes, the masses
//     are the ones before the step (the epilogue does not touch them when nstop > 1);
//   else xmassfract of the masses the epilogue stored < minmass                            -> :681, no call: :702 finds
//     itra1 = -999999999;
//   else                                                                                   -> :702, contributes with the masses
//     after deposition and decay.
// xmassfract is formed as epilogue_store forms it (timemanager.f90:662-666, in R), from the same stored values.
template <typename R, typename H>
__global__ void __launch_bounds__(256) k_initcond(Args<H> A, View<R> V, Parts<R> P, const unsigned char *__restrict__ key, unsigned char notdue,
                                                  int dead, long long numpart) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart || key[s] == notdue || P.itra1[s] != dead) return;
  const double xt = P.xt[s], yt = P.yt[s];
  const bool left = !(xt >= 0.) || !(xt < (double)(R)V.nxmin1) || !(yt >= 0.) || !(yt <= (double)(R)V.nymin1);
  const int npoint = P.npoint[s];
  if (!left && V.mdomainfill == 0 && V.mquasilag == 0) {
    const int kr = release_index(V, V.numpoint > 1 ? npoint : 1);
    const R npart_r = (R)V.rel_npart[kr];
    R xmassfract = (R)0;
    for (int ks = 0; ks < V.nspec; ks++) {
      const R xmr = V.rel_xmass[(size_t)ks * V.numpoint + kr];
      if (xmr > (R)0) xmassfract = m_max(xmassfract, npart_r * P.xmass1[(size_t)ks * P.cap + s] / xmr);
    }
    if (xmassfract < (R)0.0001) return;   // minmass, par_mod.f90:213
  }
  const PackRho<R, H> rho{V.r2, V.nx, V.nz, V.m2};
  ic_particle<H>(A, V.height, rho, xt, yt, (H)P.zt[s], npoint, P.xmass1 + s, (size_t)P.cap);
}

// timemanager.f90:735-737: every storage space with itra1 = itime.  Whole blocks, no early return: wave_kernel_add needs
// every lane of the wave.  The two level searches read the block's copies of height and outheight in LDS (from device memory
// each probe is a dependent round trip), as k_conccalc's do.
template <typename R, typename H, int MAXNZ /* the engine's limit of nz and numzgrid */>
__global__ void __launch_bounds__(256) k_initcond_finish(Args<H> A, View<R> V, Parts<R> P, long long numpart, int itime) {
  __shared__ H hgt[MAXNZ];
  __shared__ H outh[MAXNZ];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = (H)V.height[k];
  for (int k = threadIdx.x; k < A.numzgrid; k += blockDim.x) outh[k] = A.outheight[k];
  __syncthreads();
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  Hit<H> h;
  bool active = s < numpart && P.itra1[s] == itime;
  if (active) {
    const PackRho<R, H> rho{V.r2, V.nx, V.nz, V.m2};
    active = ic_locate<H>(A, hgt, outh, rho, P.xt[s], P.yt[s], (H)P.zt[s], P.npoint[s], h);
  }
  const long long c0 = active ? ic_cell(A, h) : kNoCell, sstride = (long long)A.numxgrid * A.numygrid * A.numzgrid;
  const int dix = active ? h.dix : 1, djy = active ? h.djy : 1;
  for (int k = 0; k < A.nspec; k++) {
    H t[4] = {(H)0, (H)0, (H)0, (H)0};
    if (active) {
      const H m = (H)P.xmass1[(size_t)k * P.cap + s];
      for (int q = 0; q < 4; q++)
        if (h.on[q]) t[q] = ic_value(h, m, q);
    }
    wave_kernel_add<H>(A.init_cond + sstride * k, c0, A.numxgrid, dix, djy, t[0], t[1], t[2], t[3]);
  }
}
#endif

}  // namespace ic
FPX_TU_CLOSE
}  // namespace fpx
