// Device side of fpx_calcpar_gfs: the boundary-layer parameters of the reference's calcpar for NCEP GFS fields -- the
// GRIBFILE_CENTRE_NCEP branches of src/calcpar.f90:76-265, obukhov.f90 and richardson.f90, with scalev.f90 and ew.f90 -- from
// the pressure-level arrays uuh, vvh, tth, qvh, ps, tt2, td2, akz, bkz that fpx_verttransform_gfs has left on the device.
// The plan is k_calcpar's (fpx_calcpar.hpp): one lane per grid column, consecutive lanes own consecutive ix, arithmetic in the
// host's real kind H with FMA contraction off, log / x**y / sqrt from the device's libm (vt::M<H>).
//
// The NCEP branch is reproduced as it is written.  What differs from the ECMWF branch, each item with its place:
//  * llev of calcpar (calcpar.f90:109-116): the last i with ps < akz(i), plus 1; nuvz-1 where that exceeds nuvz.  It can be 1.
//    obukhov gets tth(llev) and plev = akz(llev); the akm / bkm average of the ECMWF branch (obukhov.f90:56-60) is not used.
//  * llev of richardson (richardson.f90:73-86): computed again, with the extra `llev == 1 -> 2`.  The two values differ in the
//    columns with ps >= akz(1).
//  * richardson's level loop starts at its llev (:107-112); the reference wind stays ulev(2), vlev(2) whatever llev is
//    (:131,158).  When the loop runs out, k = nuvz (:143) and the 20-step refinement reads k-1.
//  * the mixing height is the GRIB file's (calcpar.f90:145-149): richardson's h goes to a dummy and feeds only wstar (and the
//    excess temperature of its iterations) and hmixplus.  hmix out = the host's raw hmix + min(excessoro, hmixplus) with
//    lsubgrid = 1, clamped to hmixmin / hmixmax (:156-166).
//  * the tropopause (:198-257): zlev is built from calcpar's llev upward, starting at zold = 0 with the 2 m virtual
//    temperature at ps; the kzmin search starts at llev.  A column where the criterion never fires keeps the previous value of
//    the slot's tropopause buffer (zero at first use), as for ECMWF.
//  * kzmin (:232-238) is not reset per column in the reference: a column none of whose levels reaches altmin would search
//    from the previous column's kzmin.  Here such a column searches from llev.  Real GFS columns reach 30 km and more; the
//    test inputs are checked to have no such column, so the difference is never exercised.
// richardson also evaluates f_qvsat per level (rh, rhold, rhl: :124,139,156); nothing reads them, they are left out.
// Not computed here: the dry-deposition velocities (calcpar.f90:171-189; fpx_getvdep or the host's vdep) and calcpv (:266).
//
// The column body calcpar_gfs_column compiles as host code too (FPX_CPG_HOST; tests/calcpar_gfs_host.cpp).
#pragma once
#ifndef FPX_CPG_HOST
#include "fpx_tu.hpp"
#include <hip/hip_runtime.h>
#include "fpx_verttransform.hpp"
#define FPX_CPG_FN __host__ __device__ __forceinline__
#else
#define FPX_CPG_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif
#if defined(__clang__)
#define FPX_CPG_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define FPX_CPG_NOCONTRACT
#endif
#include <cmath>
#include <cstddef>

namespace fpx {
FPX_TU_OPEN
namespace cpg {

#define GK(x) ((H)(x))

#ifdef FPX_CPG_HOST
template <typename H> struct HostM;
template <> struct HostM<float> {
  static float log(float x) { return ::logf(x); }
  static float pow(float x, float y) { return ::powf(x, y); }
  static float sqrt(float x) { return ::sqrtf(x); }
};
template <> struct HostM<double> {
  static double log(double x) { return ::log(x); }
  static double pow(double x, double y) { return ::pow(x, y); }
  static double sqrt(double x) { return ::sqrt(x); }
};
#endif

template <typename H>
FPX_CPG_FN H absv(H v) { return v < GK(0.) ? -v : v; }

// ew.f90:4-29, the text of vt::ew over the math of the caller
template <typename H, typename MM>
FPX_CPG_FN H ew(H x) {
  FPX_CPG_NOCONTRACT
  H y = GK(373.16) / x;
  H a = GK(-7.90298) * (y - GK(1.));
  a = a + (GK(5.02808) * GK(0.43429) * MM::log(y));
  H c = (GK(1.) - (GK(1.) / y)) * GK(11.344);
  c = GK(-1.) + MM::pow(GK(10.), c);
  c = GK(-1.3816) * c / GK(1.e7);
  H d = (GK(1.) - y) * GK(3.49149);
  d = GK(-1.) + MM::pow(GK(10.), d);
  d = GK(8.1328) * d / GK(1.e3);
  y = a + c + d;
  return GK(101324.6) * MM::pow(GK(10.), y);
}

// One column: level k (1-based) of a 3-D array f is f[o + stride*(k-1)]; zlev is scratch with the same addressing.
template <typename H>
struct Col {
  const H *uuh, *vvh, *tth, *qvh, *akz, *bkz;
  H *zlev;
  size_t o, stride;
  int nuvz, lsubgrid;
  H ps, tt2, td2, surfstr, sshf, hmix, excessoro, ylat;
};
template <typename H>
struct ColOut {
  H ustar, wstar, oli, hmix, tropopause;
  int have_tropopause;         // 0: the criterion never fired, tropopause is not to be written
  int llev, llev_ri, kbreak, istep, iter;   // the record: both llev, richardson's last k, refinement step, iterations
};

template <typename H, typename MM>
FPX_CPG_FN void calcpar_gfs_column(const Col<H> &C, ColOut<H> &O) {
  FPX_CPG_NOCONTRACT
  const int nuvz = C.nuvz;
  const H r_air = GK(287.05), ga = GK(9.81), cpa = GK(1004.6), karman = GK(0.40), convke = GK(2.0);
  const H konst = r_air / ga;
  const H ps = C.ps, tt2 = C.tt2, td2 = C.td2, hf = C.sshf;
#define CPG_L(f, k) (C.f[C.o + C.stride * (size_t)((k) - 1)])
  // calcpar.f90:84-95
  const H ylat = C.ylat;
  H altmin;
  if (ylat >= GK(-20.) && ylat <= GK(20.)) altmin = GK(5000.);
  else if (ylat > GK(20.) && ylat < GK(40.)) altmin = GK(2500.) + (GK(40.) - ylat) * GK(125.);
  else if (ylat > GK(-40.) && ylat < GK(-20.)) altmin = GK(2500.) + (GK(40.) + ylat) * GK(125.);
  else altmin = GK(2500.);
  const H tv2 = tt2 * (GK(1.) + GK(0.378) * ew<H, MM>(td2) / ps);
  const H rhoa = ps / (r_air * tv2);
  // 1) scalev.f90
  H ust = MM::sqrt(absv(C.surfstr) / rhoa);
  if (ust <= GK(1.e-8)) ust = GK(1.e-8);
  // first level above ground: calcpar.f90:111-116 and richardson.f90:77-84
  int last = 0;
  for (int i = 1; i <= nuvz; i++)
    if (ps < C.akz[i - 1]) last = i;
  int llev = last + 1, llr = last + 1;
  if (llev > nuvz) llev = nuvz - 1;
  if (llr == 1) llr = 2;
  if (llr > nuvz) llr = nuvz - 1;
  // 2) obukhov.f90, NCEP: tlev = tth(llev), plev = akz(llev)
  H ol;
  {
    const H plev = C.akz[llev - 1];
    const H theta = CPG_L(tth, llev) * MM::pow(GK(100000.) / plev, r_air / cpa);
    const H thetastar = hf / (rhoa * cpa * ust);
    if (absv(thetastar) > GK(1.e-10)) ol = theta * (ust * ust) / (karman * ga * thetastar); else ol = GK(9999);
    if (ol > GK(9999.)) ol = GK(9999.);
    if (ol < GK(-9999.)) ol = GK(-9999.);
  }
  O.ustar = ust;
  O.oli = ol != GK(0.) ? GK(1.) / ol : GK(99999.);
  O.llev = llev; O.llev_ri = llr;
  // 3) richardson.f90, NCEP: the loop starts at llr, the reference wind is level 2's
  H hm, wst, hmixplus;
  {
    const H ric = GK(0.25), b = GK(100.), bs = GK(8.5);
    const H u2 = CPG_L(uuh, 2), v2 = CPG_L(vvh, 2);
    H excess = GK(0.);
    for (int iter = 1;; iter++) {
      H pold = ps, tvold = tv2, zold = GK(2.0);
      const H zref = zold;
      const H thetaref = tvold * MM::pow(GK(100000.) / pold, r_air / cpa) + excess;
      H thetaold = thetaref, z = GK(0.), theta = GK(0.);
      int k;
      for (k = llr; k <= nuvz; k++) {
        const H pint = C.akz[k - 1] + C.bkz[k - 1] * ps;
        const H tv = CPG_L(tth, k) * (GK(1.) + GK(0.608) * CPG_L(qvh, k));
        if (absv(tv - tvold) > GK(0.2)) z = zold + konst * MM::log(pold / pint) * (tv - tvold) / MM::log(tv / tvold);
        else z = zold + konst * MM::log(pold / pint) * tv;
        theta = tv * MM::pow(GK(100000.) / pint, r_air / cpa);
        const H du = CPG_L(uuh, k) - u2, dv = CPG_L(vvh, k) - v2;
        H den = du * du + dv * dv + b * (ust * ust);
        if (den < GK(0.1)) den = GK(0.1);
        const H ri = ga / thetaref * (theta - thetaref) * (z - zref) / den;
        if (ri > ric && thetaold < theta) break;
        tvold = tv; pold = pint; thetaold = theta; zold = z;
      }
      if (k > nuvz) k = nuvz;                  // :143
      const H uk = CPG_L(uuh, k), uk1 = CPG_L(uuh, k - 1), vk = CPG_L(vvh, k), vk1 = CPG_L(vvh, k - 1);
      H zl = zold, ul = uk1, vl = vk1, zl1 = zold, theta1 = thetaold, zl2 = zold, theta2 = thetaold;
      int i;
      for (i = 1; i <= 20; i++) {
        const H fr = (H)i / GK(20.);
        zl = zold + fr * (z - zold);
        ul = uk1 + fr * (uk - uk1);
        vl = vk1 + fr * (vk - vk1);
        const H thetal = thetaold + fr * (theta - thetaold);
        H den = (ul - u2) * (ul - u2) + (vl - v2) * (vl - v2) + b * (ust * ust);
        if (den < GK(0.1)) den = GK(0.1);
        const H ril = ga / thetaref * (thetal - thetaref) * (zl - zref) / den;
        zl2 = zl; theta2 = thetal;
        if (ril > ric) break;
        zl1 = zl; theta1 = thetal;
      }
      hm = zl;
      const H thetam = GK(0.5) * (theta1 + theta2);
      const H wspeed = MM::sqrt(ul * ul + vl * vl);
      const H bvfsq = (ga / thetam) * (theta2 - theta1) / (zl2 - zl1);
      if (bvfsq <= GK(0.)) hmixplus = GK(9999.); else hmixplus = wspeed / MM::sqrt(bvfsq) * convke;
      O.kbreak = k; O.istep = i; O.iter = iter;
      if (hf < GK(0.)) {
        wst = MM::pow(-hm * ga / thetaref * hf / cpa, GK(0.333));
        excess = -bs * hf / cpa / wst;
        if (iter < 3) continue;
      } else wst = GK(0.);
      break;
    }
  }
  // calcpar.f90:156-166: richardson's h is dropped, the mixing height is the GRIB file's
  H subsceff = GK(0.0);
  if (C.lsubgrid == 1) { subsceff = C.excessoro; if (hmixplus < subsceff) subsceff = hmixplus; }
  H hmx = C.hmix + subsceff;
  if (hmx < GK(100.)) hmx = GK(100.);         // hmixmin, hmixmax: par_mod.f90:77
  if (hmx > GK(4500.)) hmx = GK(4500.);
  O.hmix = hmx; O.wstar = wst;
  // thermal tropopause, calcpar.f90:198-257, from llev
  {
    H tvold = tv2, pold = ps, zold = GK(0.);
    int kzmin = llev;
    bool have = false;
    for (int kz = llev; kz <= nuvz; kz++) {
      const H pint = C.akz[kz - 1] + C.bkz[kz - 1] * ps;
      const H tv = CPG_L(tth, kz) * (GK(1.) + GK(0.608) * CPG_L(qvh, kz));
      H z;
      if (absv(tv - tvold) > GK(0.2)) z = zold + konst * MM::log(pold / pint) * (tv - tvold) / MM::log(tv / tvold);
      else z = zold + konst * MM::log(pold / pint) * tv;
      CPG_L(zlev, kz) = z;
      if (!have && z >= altmin) { kzmin = kz; have = true; }
      tvold = tv; pold = pint; zold = z;
    }
    O.have_tropopause = 0;
    O.tropopause = GK(0.);
    for (int kz = kzmin; kz <= nuvz && !O.have_tropopause; kz++) {
      const H zk = CPG_L(zlev, kz), tk = CPG_L(tth, kz);
      for (int lz = kz + 1; lz <= nuvz; lz++) {
        const H zz = CPG_L(zlev, lz);
        if (zz - zk > GK(2000.)) {
          if ((tk - CPG_L(tth, lz)) / (zz - zk) < GK(0.002)) { O.tropopause = zk; O.have_tropopause = 1; }
          break;
        }
      }
    }
  }
#undef CPG_L
}

#ifndef FPX_CPG_HOST
template <typename H>
struct Args {
  vt::Geo<H> G;
  vt::In<H> I;                 // uuh, vvh, tth, qvh (nuvz levels), ps, tt2, td2, akz, bkz on the device, host layout
  const H *surfstr, *sshf, *excessoro;
  int lsubgrid;
  H *zlev;                     // scratch [nuvz][nymax][nxmax]
  H *ustar, *wstar, *oli, *tropopause;   // out, host layout (0:nxmax-1,0:nymax-1)
  H *hmix;                     // in: hmix(0,0,1,n) as readwind_gfs left it; out: calcpar's
};

template <typename H>
__global__ void __launch_bounds__(256) k_calcpar_gfs(Args<H> A) {
  const vt::Geo<H> &G = A.G;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= G.nx * G.ny) return;
  const int ix = c % G.nx, jy = c / G.nx;
  const size_t i2 = G.at2(ix, jy);
  Col<H> C;
  C.uuh = A.I.uuh; C.vvh = A.I.vvh; C.tth = A.I.tth; C.qvh = A.I.qvh; C.akz = A.I.akz; C.bkz = A.I.bkz;
  C.zlev = A.zlev;
  C.o = G.at(ix, jy, 1); C.stride = (size_t)G.nxmax * (size_t)G.nymax;
  C.nuvz = G.nuvz; C.lsubgrid = A.lsubgrid;
  C.ps = A.I.ps[i2]; C.tt2 = A.I.tt2[i2]; C.td2 = A.I.td2[i2];
  C.surfstr = A.surfstr[i2]; C.sshf = A.sshf[i2]; C.hmix = A.hmix[i2];
  C.excessoro = A.lsubgrid == 1 ? A.excessoro[i2] : GK(0.);
  C.ylat = G.ylat0 + (H)jy * G.dy;
  ColOut<H> O;
  calcpar_gfs_column<H, vt::M<H>>(C, O);
  A.ustar[i2] = O.ustar; A.wstar[i2] = O.wstar; A.oli[i2] = O.oli; A.hmix[i2] = O.hmix;
  if (O.have_tropopause) A.tropopause[i2] = O.tropopause;
}
#endif

#undef GK

}  // namespace cpg
FPX_TU_CLOSE
}  // namespace fpx
