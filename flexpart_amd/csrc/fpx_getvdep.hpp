// Device side of fpx_getvdep: the dry-deposition velocities the reference computes inside calcpar (src/calcpar.f90:171-189)
// with getvdep.f90, getrb.f90, getrc.f90, raerod.f90, psih.f90 and partdep.f90, from ustar and oli (which fpx_calcpar has
// just written on the device), ps, tt2, td2 (of fpx_verttransform_ecmwf) and the four 2-D fields ssr, lsprec, convprec, sd.
// The land-use inventory (xlanduse) and the resistance tables stay the host's: they are read once at start-up and come in
// through fpx_getvdep_init as plain arrays of com_mod.  A nested grid (getvdep_nests.f90) runs the same kernel on its own
// view: nxn, nyn, strides nxmaxn, nymaxn, xlandusen(:,:,:,l) of fpx_getvdep_nest_init, and a season table over its nyn rows.
// One lane per grid column; consecutive lanes own consecutive ix, so every read of a 2-D field and of one class plane of
// xlanduse is one contiguous row segment.  The small tables (z0, ri, rac, rcl/rgs/rlu, the per-species constants, vset,
// schmi, fract) sit in LDS, loaded once per block.  z0(7), which calcpar.f90:174 overwrites per column, is lane-private and
// never written to the shared table.  The class loop adds ra*slanduse and vd*slanduse in the reference's order j = 1..numclass.
// The season (getvdep.f90:51-77) depends on the row and the wind-field time only: the host side computes lseason[jy].
// Arithmetic in the host's real kind H with FMA contraction off; log, log10, exp, x**y come from the device's libm.
#pragma once
#include "fpx_tu.hpp"
#include <hip/hip_runtime.h>
#include "fpx_verttransform.hpp"

namespace fpx {
FPX_TU_OPEN
namespace gv {

#ifndef CK
#define CK(x) ((H)(x))
#endif

constexpr int kMaxSpec = 5;          // FPX_MAXSPEC (par_mod.f90:211 maxspec): the lane-private rb, rc, vdepo

template <typename H> __device__ __forceinline__ H m_log10(H x);
template <> __device__ __forceinline__ float m_log10<float>(float x) { return ::log10f(x); }
template <> __device__ __forceinline__ double m_log10<double>(double x) { return ::log10(x); }

// the small tables of com_mod, packed in this order (Fortran layouts kept): offsets in elements of H
struct Layout {
  int numclass, ni, maxspec;
  __host__ __device__ int z0() const { return 0; }                                   // z0(numclass)
  __host__ __device__ int ri() const { return numclass; }                            // ri(5,numclass)
  __host__ __device__ int rac() const { return ri() + 5 * numclass; }                // rac(5,numclass)
  __host__ __device__ int rcl() const { return rac() + 5 * numclass; }               // rcl(maxspec,5,numclass)
  __host__ __device__ int rgs() const { return rcl() + maxspec * 5 * numclass; }
  __host__ __device__ int rlu() const { return rgs() + maxspec * 5 * numclass; }
  __host__ __device__ int spec() const { return rlu() + maxspec * 5 * numclass; }    // rm, reldiff, henry, f0, density, dryvel (maxspec each)
  __host__ __device__ int vset() const { return spec() + 6 * maxspec; }              // vset, schmi, fract (maxspec,ni)
  __host__ __device__ int total() const { return vset() + 3 * maxspec * ni; }
};

template <typename H>
struct Args {
  int nx, ny, nxmax, nymax, nspec;
  Layout T;
  const H *tables;                   // Layout::total() values
  const H *xlanduse;                 // (0:nxmax-1,0:nymax-1,numclass)
  const H *ustar, *oli, *ps, *tt2, *td2, *ssr, *lsprec, *convprec, *sd;   // (0:nxmax-1,0:nymax-1)
  const unsigned char *lseason;      // [ny], 1..5
  H *vdep;                           // out: (0:nxmax-1,0:nymax-1,nspec)
};

// psih.f90:39-56; the argument l is clamped in place (:39-43)
template <typename H>
__device__ __forceinline__ H psih(H z, H &l) {
#pragma clang fp contract(off)
  typedef vt::M<H> M;
  const H a = CK(1.), b = CK(0.667), c = CK(5.), d = CK(0.35), eps = CK(1.e-20);
  if (l >= CK(0.) && l < eps) l = eps;
  else if (l < CK(0.) && l > CK(-1.) * eps) l = CK(-1.) * eps;
  if (m_log10<H>(z) - m_log10<H>(fabs(l)) < m_log10<H>(eps)) return CK(0.);
  const H zeta = z / l;
  if (zeta > CK(0.))
    return -M::pow(CK(1.) + CK(0.667) * a * zeta, CK(1.5)) - b * (zeta - c / d) * M::exp(-d * zeta) - b * c / d + CK(1.);
  const H x = M::pow(CK(1.) - CK(16.) * zeta, CK(.25));
  return CK(2.) * M::log((CK(1.) + x * x) / CK(2.));
}

// raerod.f90:43 (href, karman: par_mod.f90:76)
template <typename H>
__device__ __forceinline__ H raerod(H &l, H ust, H z0) {
#pragma clang fp contract(off)
  const H href = CK(15.), karman = CK(0.40);
  const H lg = vt::M<H>::log(href / z0);
  const H p1 = psih<H>(href, l);
  const H p2 = psih<H>(z0, l);
  return (lg - p1 + p2) / (karman * ust);
}

template <typename H>
__global__ void __launch_bounds__(256) k_getvdep(Args<H> A) {
#pragma clang fp contract(off)
  typedef vt::M<H> M;
  extern __shared__ __align__(16) unsigned char gv_lds[];
  H *S = reinterpret_cast<H *>(gv_lds);
  const Layout T = A.T;
  for (int i = threadIdx.x; i < T.total(); i += blockDim.x) S[i] = A.tables[i];
  __syncthreads();
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.nx * A.ny) return;
  const int ix = c % A.nx, jy = c / A.nx;
  const size_t i2 = (size_t)ix + (size_t)A.nxmax * (size_t)jy, plane = (size_t)A.nxmax * (size_t)A.nymax;
  const int nc = T.numclass, ni = T.ni, ms = T.maxspec, nspec = A.nspec;
  const H *z0 = S + T.z0(), *ri = S + T.ri(), *rac = S + T.rac(), *rcl = S + T.rcl(), *rgs = S + T.rgs(), *rlu = S + T.rlu();
  const H *rm = S + T.spec(), *reldiff = rm + ms, *henry = reldiff + ms, *f0 = henry + ms, *density = f0 + ms, *dryvel = density + ms;
  const H *vset = S + T.vset(), *schmi = vset + ms * ni, *fract = schmi + ms * ni;
  const H ga = CK(9.81), karman = CK(0.40);
  // calcpar.f90:174-183
  const H ust = A.ustar[i2], temp = A.tt2[i2], pa = A.ps[i2], gr = A.ssr[i2], snow = A.sd[i2];
  const H z0water = CK(0.016) * ust * ust / ga;                 // z0(7), this column's
  const H rh = vt::ew<H>(A.td2[i2]) / vt::ew<H>(temp);
  H L = CK(1.) / A.oli[i2];
  const H rr = A.lsprec[i2] + A.convprec[i2];
  const int lseason = A.lseason[jy];
  // getvdep.f90:81-101
  const H diffh2o = CK(2.11e-5) * M::pow(temp / CK(273.15), CK(1.94)) * (CK(101325.) / pa);
  const H tc = temp - CK(273.15);
  H myl;
  if (tc < CK(0.)) myl = (CK(1.718) + CK(0.0049) * tc - CK(1.2e-05) * (tc * tc)) * CK(1.e-05);
  else myl = (CK(1.718) + CK(0.0049) * tc) * CK(1.e-05);
  const H rhoa = pa / (CK(287.) * temp);
  const H nyl = myl / rhoa;
  H vdepo[kMaxSpec], rb[kMaxSpec];
#pragma unroll
  for (int i = 0; i < kMaxSpec; i++) { vdepo[i] = CK(0.); rb[i] = CK(0.); }
  // getrb.f90:36-41
#pragma unroll
  for (int i = 0; i < kMaxSpec; i++)
    if (i < nspec && reldiff[i] > CK(0.)) {
      const H schmidt = nyl / diffh2o * reldiff[i];
      rb[i] = CK(2.0) * M::pow(schmidt / CK(0.72), CK(0.67)) / (karman * ust);
    }
  // getrc.f90:49-68, the part that does not depend on the class
  const bool stom = tc > CK(0.) && tc < CK(40.);
  const H rsfac = stom ? (CK(1.) + (CK(200.) / (gr + CK(0.1))) * (CK(200.) / (gr + CK(0.1)))) : CK(0.);
  const H rstc = stom ? CK(400.) / (tc * (CK(40.) - tc)) : CK(0.);
  const bool wet = rh > CK(0.9) || rr > CK(0.);
  const H rdc = CK(100.) * (CK(1.) + CK(1000.) / (gr + CK(10.)));
  const H corr = CK(1000.) * M::exp(CK(-1.) * tc - CK(4.));
  const bool snowy = snow > CK(0.001);
  H raquer = CK(0.);
  for (int j = 1; j <= nc; j++) {                               // getvdep.f90:118-161, in the reference's order
    H sl;
    if (snowy) sl = j == 12 ? CK(1.) : CK(0.);
    else sl = A.xlanduse[i2 + plane * (size_t)(j - 1)];
    if (!(sl > CK(1.e-5))) continue;
    const H ra = raerod<H>(L, ust, j == 7 ? z0water : z0[j - 1]);
    raquer = raquer + ra * sl;
    const int ij = (lseason - 1) + 5 * (j - 1);
    H rs = stom ? ri[ij] * rsfac * rstc : CK(1.E25);
    if (wet) rs = rs * CK(3.);
#pragma unroll
    for (int i = 0; i < kMaxSpec; i++) {
      if (i >= nspec || !(reldiff[i] > CK(0.))) continue;
      const H rsm = rs * reldiff[i] + rm[i];
      H rluc = rlu[i + ms * ij] + corr;
      const H rclc = rcl[i + ms * ij] + corr;
      const H rgsc = rgs[i + ms * ij] + corr;
      if (rr > CK(0.)) {                                        // getrc.f90:87-93: rain before dew
        const H rluo = CK(1.) / (CK(1.) / CK(1000.) + CK(1.) / (CK(3.) * rluc));
        rluc = CK(1.) / (CK(1.) / (CK(3.) * rluc) + CK(1.e-7) * henry[i] + f0[i] / rluo);
      } else if (rh > CK(0.9)) {
        const H rluo = CK(1.) / (CK(1.) / CK(3000.) + CK(1.) / (CK(3.) * rluc));
        rluc = CK(1.) / (CK(1.) / (CK(3.) * rluc) + CK(1.e-7) * henry[i] + f0[i] / rluo);
      }
      H rc = CK(1.) / (CK(1.) / rsm + CK(1.) / rluc + CK(1.) / (rdc + rclc) + CK(1.) / (rac[ij] + rgsc));
      if (rc < CK(10.)) rc = CK(10.);
      H vd;                                                     // getvdep.f90:150-158
      if (ra + rb[i] + rc > CK(0.)) vd = CK(1.) / (ra + rb[i] + rc); else vd = CK(9.999);
      vdepo[i] = vdepo[i] + vd * sl;
    }
  }
  // partdep.f90:67-102
  const H lgeps = m_log10<H>(CK(1.e-5));
#pragma unroll
  for (int i = 0; i < kMaxSpec; i++) {
    if (i >= nspec || !(density[i] > CK(0.))) continue;
    for (int j = 0; j < ni; j++) {
      const H vs = vset[i + ms * j];
      H vdepj;
      if (ust > CK(1.e-5)) {
        const H stokes = vs / ga * ust * ust / nyl;
        const H alpha = CK(-3.) / stokes;
        H rdp;
        if (alpha <= lgeps) rdp = CK(1.) / (schmi[i + ms * j] * ust);
        else rdp = CK(1.) / ((schmi[i + ms * j] + M::pow(CK(10.), alpha)) * ust);
        vdepj = vs + CK(1.) / (raquer + rdp + raquer * rdp * vs);
      } else vdepj = vs;
      vdepo[i] = vdepo[i] + vdepj * fract[i + ms * j];
    }
  }
  // getvdep.f90:178-183, calcpar.f90:185-187
#pragma unroll
  for (int i = 0; i < kMaxSpec; i++) {
    if (i >= nspec) continue;
    if (reldiff[i] < CK(0.) && density[i] < CK(0.) && dryvel[i] > CK(0.)) vdepo[i] = dryvel[i];
    A.vdep[i2 + plane * (size_t)i] = vdepo[i];
  }
}

}  // namespace gv
FPX_TU_CLOSE
}  // namespace fpx
