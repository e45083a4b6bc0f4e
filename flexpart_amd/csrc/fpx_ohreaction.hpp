// OH chemistry (SPECIES files with ohcconst > 0): gethourlyOH.f90:40-142 (timemanager.f90:212-216) on the engine's host side and
// ohreaction.f90:47-153 (timemanager.f90:171-172) on the device.
//
// Host side (oh::Hourly<H>, plain C++ in the host's real kind H with libm -- the functions a flang build of the reference calls,
// so OH_hourly and memOHtime are the reference's bit for bit): the three-branch state machine of gethourlyOH with caldate.f90,
// zenithangle.f90 and photo_O1D.f90.  The reference evaluates the zenith angle and the photolysis rate for every kz; they depend
// on the column only and are formed once per column here.  Its quirks are kept: the first call sets memOHtime(1) = 0 whatever
// itime is and forms the second date as bdate + ldirect*real(1./24., dp) with the quotient in the default kind (:104); later
// calls use bdate + memOHtime(2)/86400._dp (:61); one call advances the pair by at most one hour; caldate may move the date it is
// handed (caldate.f90:44-47), and the moved date is what the following calls see.
//
// Device side, two kernels.  k_oh_blend forms the time blend of ohreaction.f90:124-126 per cell of the OH grid -- the weight is
// the same for every particle -- in the reference's order, so a cell holds what the reference gives every particle in it.
// k_ohreaction runs oh_particle() on one lane per storage space 1..numpart:
//   * nest pick with the strict inequalities of :65-71, highest nest first; ix, jy from the nest coordinates inside a nest;
//   * temp = tt(ix,jy,indz,n) reads the MOTHER grid's tt with those nest indices (:133) -- reproduced, not repaired (fpx_oh_init
//     refuses a nest with more columns than the mother grid, where the reference reads padding or out of bounds);
//   * n = 1 or 2 by |memtime(k) - nint(itime - 0.5*ltsample)| (:85-87) and is used as the slot itself, not through memind;
//   * indz is find_level (the comparisons of :89-95); where no level lies above the particle the reference keeps the previous
//     particle's indz, the device takes nz-1;
//   * xlon, ylat are formed in double, rounded to H, xlon wrapped at 180 (:101-105);
//   * OHx, OHy, OHz (the minloc(abs(..)) picks of :108-119, first index on a tie) by bisection over the strictly increasing
//     lonOH, latOH, altOHtop, then the reference's own abs(a(i) - x) on the two bracketing entries, the lower index unless the
//     upper is strictly smaller (check_axis() makes sure at init that the rounded differences are strictly monotone on
//     either side of the minimum); altOHtop (:114-117) is formed once at init.  Its last two entries are equal whatever
//     altOH is (both are altOH(nzOH) + 0.5*(altOH(nzOH) - altOH(nzOH-1))), so minloc's first-index rule never picks level
//     nzOH: the search looks at the first nzOH-1 entries;
//   * the reaction of :128-151 in H, operation order kept, FMA contraction off; tiny is that of the type xmass1 is kept in;
//     ohreacted, m, h and ldeltat are computed by the reference and never used, and are left out.
// The reference also runs over terminated storage spaces, whose mass nobody reads; the device skips itra1 = FPX_DEAD.  Every
// index is clamped into its array before a load; a live particle whose ix, jy fall outside the mother grid is left untouched
// and counted (the only atomic of the kernel, on a path no valid run takes).
// oh_particle and check_axis compile as host code too (FPX_OH_HOST; tests/ohreaction_host.cpp).
#pragma once
#ifndef FPX_OH_HOST
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#define FPX_OH_FN __device__ __forceinline__
#else
#define FPX_OH_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif
#if defined(__clang__)
#define FPX_OH_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define FPX_OH_NOCONTRACT
#endif
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <limits>
#include <vector>

namespace fpx {
FPX_TU_OPEN
namespace oh {

constexpr int kOhMaxSpec = 5;     // FPX_MAXSPEC
constexpr int kOhMaxNests = 4;    // FPX_MAXNESTS
constexpr int kOhDead = -999999999;

// ---- host side: gethourlyOH -----------------------------------------------------------------------------------------
template <typename H> struct Lm;
template <> struct Lm<float> {
  static float sin(float v) { return ::sinf(v); }
  static float cos(float v) { return ::cosf(v); }
  static float asin(float v) { return ::asinf(v); }
  static float exp(float v) { return ::expf(v); }
  static float log(float v) { return ::logf(v); }
};
template <> struct Lm<double> {
  static double sin(double v) { return ::sin(v); }
  static double cos(double v) { return ::cos(v); }
  static double asin(double v) { return ::asin(v); }
  static double exp(double v) { return ::exp(v); }
  static double log(double v) { return ::log(v); }
};

// caldate.f90:42-78; the default-kind arithmetic of its integer formulas in H; juldate may be moved (:44-47)
template <typename H>
inline void caldate(double &juldate, int &yyyymmdd, int &hhmiss) {
  FPX_OH_NOCONTRACT
  const int igreg = 2299161;
  int julday = (int)juldate;
  if ((juldate - (double)julday) * 86400. >= 86399.5) {
    juldate = juldate + juldate - (double)julday - 86399.5 / 86400.;
    julday = (int)juldate;
  }
  int ja;
  if (julday >= igreg) {
    const int jalpha = (int)(((H)(julday - 1867216) - (H)0.25) / (H)36524.25);
    ja = julday + 1 + jalpha - (int)((H)0.25 * (H)jalpha);
  } else ja = julday;
  const int jb = ja + 1524;
  const int jc = (int)((H)6680. + ((H)(jb - 2439870) - (H)122.1) / (H)365.25);
  const int jd = 365 * jc + (int)((H)0.25 * (H)jc);
  const int je = (int)((H)(jb - jd) / (H)30.6001);
  const int dd = jb - jd - (int)((H)30.6001 * (H)je);
  int mm = je - 1;
  if (mm > 12) mm = mm - 12;
  int yyyy = jc - 4715;
  if (mm > 2) yyyy = yyyy - 1;
  if (yyyy <= 0) yyyy = yyyy - 1;
  yyyymmdd = 10000 * yyyy + 100 * mm + dd;
  const double fr = juldate - (double)julday;
  int hh = (int)(24. * fr);
  int mi = (int)(1440. * fr - 60. * (double)hh);
  int ss = (int)std::lround(86400. * fr - 3600. * (double)hh - 60. * (double)mi);
  if (ss == 60) { ss = 0; mi = mi + 1; }
  if (mi == 60) { mi = 0; hh = hh + 1; }
  hhmiss = 10000 * hh + 100 * mi + ss;
}

inline int month_of(int yyyymmdd) { return (yyyymmdd - (yyyymmdd / 10000) * 10000) / 100; }

// zenithangle.f90:44-74
template <typename H>
inline H zenithangle(H ylat, H xlon, double &jul) {
  FPX_OH_NOCONTRACT
  typedef Lm<H> M;
  int yyyymmdd, hhmmss;
  caldate<H>(jul, yyyymmdd, hhmmss);
  const int jjjj = yyyymmdd / 10000, mm = yyyymmdd / 100 - jjjj * 100, id = yyyymmdd - jjjj * 10000 - mm * 100;
  const int iu = hhmmss / 10000, minute = hhmmss / 100 - 100 * iu;
  int ndaynum = 31 * (mm - 1) + id;
  if (mm > 2) ndaynum = ndaynum - (int)((H)0.4 * (H)mm + (H)2.3);
  if (mm > 2 && jjjj / 4 * 4 == jjjj) ndaynum = ndaynum + 1;
  const H pi = (H)3.1415927;
  const H rnum = (H)2. * pi * (H)ndaynum / (H)365.;
  const H rylat = pi * ylat / (H)180.;
  const H ttime = (H)iu + (H)minute / (H)60.;
  const H dekl = (H)0.396 + (H)3.631 * M::sin(rnum) + (H)0.038 * M::sin((H)2. * rnum) + (H)0.077 * M::sin((H)3. * rnum) -
                 (H)22.97 * M::cos(rnum) - (H)0.389 * M::cos((H)2. * rnum) - (H)0.158 * M::cos((H)3. * rnum);
  const H rdekl = pi * dekl / (H)180.;
  const H eq = ((H)0.003 - (H)7.343 * M::sin(rnum) - (H)9.47 * M::sin((H)2. * rnum) - (H)0.329 * M::sin((H)3. * rnum) -
                (H)0.196 * M::sin((H)4. * rnum) + (H)0.552 * M::cos(rnum) - (H)3.020 * M::cos((H)2. * rnum) -
                (H)0.076 * M::cos((H)3. * rnum) - (H)0.125 * M::cos((H)4. * rnum)) / (H)60.;
  const H sinsol = M::sin(rylat) * M::sin(rdekl) + M::cos(rylat) * M::cos(rdekl) * M::cos((ttime - (H)12. + xlon / (H)15. + eq) * pi / (H)12.);
  const H solelev = M::asin(sinsol) * (H)180. / pi;
  return (H)90. - solelev;
}

// photo_O1D.f90:38-56
template <typename H>
inline H photo_O1D(H sza) {
  FPX_OH_NOCONTRACT
  typedef Lm<H> M;
  const H zangle[11] = {(H)0., (H)10., (H)20., (H)30., (H)40., (H)50., (H)60., (H)70., (H)78., (H)86., (H)90.0001};
  const H fact_photo[11] = {(H)0.4616E-02, (H)0.4478E-02, (H)0.4131E-02, (H)0.3583E-02, (H)0.2867E-02, (H)0.2081E-02,
                            (H)0.1235E-02, (H)0.5392E-03, (H)0.2200E-03, (H)0.1302E-03, (H)0.0902E-03};
  const H pi = (H)3.1415927;
  if (!(sza < (H)90.)) return (H)0.;
  int ik = 1;
  for (int iz = 1; iz <= 10; iz++)
    if (sza >= zangle[iz - 1]) ik = iz;
  const H z1 = (H)1. / M::cos(zangle[ik - 1] * pi / (H)180.);
  const H z2 = (H)1. / M::cos(zangle[ik] * pi / (H)180.);
  const H zg = (H)1. / M::cos(sza * pi / (H)180.);
  const H dummy = (zg - z1) / (z2 - z1);
  const H f1 = M::log(fact_photo[ik - 1]);
  const H f2 = M::log(fact_photo[ik]);
  const H photo_NO2 = (H)1.45e-2 * M::exp((H)-0.4 / M::cos(sza * pi / (H)180.));
  return photo_NO2 * M::exp(f1 + (f2 - f1) * dummy);
}

// minloc(abs(a - x)), the first index of the minimum, 0-based: a plain scan (host side, once per row and column of the OH grid)
template <typename H>
inline int nearest_scan(const H *a, int n, H x) {
  int best = 0;
  H bv = std::fabs(a[0] - x);
  for (int i = 1; i < n; i++) {
    const H v = std::fabs(a[i] - x);
    if (v < bv) { bv = v; best = i; }
  }
  return best;
}

// What the bisection of oh_nearest needs from an axis (lonOH, latOH, altOHtop): strictly increasing, and every spacing more
// than four units in the last place of the largest magnitude, so that the rounded differences |a(i) - x| stay strictly
// monotone on either side of their minimum.  Returns NULL or what is wrong.
template <typename H>
inline const char *check_axis(const H *a, int n) {
  if (n < 1) return "is empty";
  H big = (H)0;
  for (int i = 0; i < n; i++) {
    if (!(a[i] - a[i] == (H)0)) return "holds a value that is not finite";
    big = std::fabs(a[i]) > big ? std::fabs(a[i]) : big;
  }
  const H ulp = std::nextafter(big, std::numeric_limits<H>::infinity()) - big;
  for (int i = 0; i + 1 < n; i++) {
    if (!(a[i + 1] > a[i])) return "does not increase strictly";
    if (!(a[i + 1] - a[i] > (H)4. * ulp)) return "has a spacing of no more than four units in the last place of its largest value";
  }
  return nullptr;
}

// altOHtop of ohreaction.f90:114-117 (nz >= 2)
template <typename H>
inline void alt_tops(const H *alt, int nz, H *top) {
  FPX_OH_NOCONTRACT
  for (int i = 2; i <= nz; i++) top[i - 2] = alt[i - 1] + (H)0.5 * (alt[i - 1] - alt[i - 2]);
  top[nz - 1] = alt[nz - 1] + (H)0.5 * (alt[nz - 1] - alt[nz - 2]);
}

enum { BR_NONE = 0, BR_ADVANCE = 1, BR_INIT = 2 };

// oh_mod as the host hands it over (fpx_oh_init), and OH_hourly / memOHtime as gethourlyOH keeps them
template <typename H>
struct Hourly {
  int nx = 0, ny = 0, nz = 0, ldirect = 1;
  double bdate = 0.;
  std::vector<H> lon, lat, alt, field, jr, lonjr, latjr;
  std::vector<H> hourly;          // OH_hourly(nx,ny,nz,2)
  H memtime[2] = {(H)0, (H)0};    // memOHtime
  std::vector<int> ijx, jjy;      // the minloc picks of gethourlyOH.f90:71-72 = :116-117 per column and row
  size_t cells() const { return (size_t)nx * ny * nz; }

  void prepare() {
    hourly.assign(2 * cells(), (H)0);
    memtime[0] = memtime[1] = (H)0;
    ijx.resize(nx); jjy.resize(ny);
    for (int i = 0; i < nx; i++) ijx[i] = nearest_scan(lonjr.data(), 360, lon[i]);
    for (int j = 0; j < ny; j++) jjy[j] = nearest_scan(latjr.data(), 180, lat[j]);
  }
  // OH_hourly(:,:,:,slot) for the date jul (which caldate may move) and its month m
  void fill(int slot, double &jul, int m) {
    FPX_OH_NOCONTRACT
    H *out = hourly.data() + (size_t)slot * cells();
    const H *jrm = jr.data() + (size_t)(m - 1) * 360 * 180;
    const H *fm = field.data() + (size_t)(m - 1) * cells();
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        const H sza = zenithangle<H>(lat[j], lon[i], jul);
        const H jrate = photo_O1D<H>(sza);
        const H ja = jrm[(size_t)jjy[j] * 360 + ijx[i]];
        for (int k = 0; k < nz; k++) {
          const size_t c = ((size_t)k * ny + j) * nx + i;
          out[c] = ja > (H)0. ? fm[c] * jrate / ja : (H)0.;
        }
      }
  }
  // gethourlyOH.f90:40-142; returns the branch taken
  int step(int itime) {
    FPX_OH_NOCONTRACT
    const H ld = (H)ldirect, t = (H)(ldirect * itime);
    if (ld * memtime[0] <= t && ld * memtime[1] > t) return BR_NONE;
    int ymd, hms;
    if (ld * memtime[1] <= t && memtime[1] != (H)0.) {
      memtime[0] = memtime[1];
      memtime[1] = memtime[0] + ld * (H)3600.;
      std::copy(hourly.begin() + cells(), hourly.end(), hourly.begin());
      double jul2 = bdate + (double)memtime[1] / 86400.;
      caldate<H>(jul2, ymd, hms);
      fill(1, jul2, month_of(ymd));
      return BR_ADVANCE;
    }
    double jul1 = bdate;
    caldate<H>(jul1, ymd, hms);
    const int m1 = month_of(ymd);
    memtime[0] = (H)0.;
    double jul2 = bdate + (double)ldirect * (double)((H)1. / (H)24.);
    caldate<H>(jul2, ymd, hms);
    const int m2 = month_of(ymd);
    memtime[1] = ld * (H)3600.;
    fill(0, jul1, m1);
    fill(1, jul2, m2);
    return BR_INIT;
  }
};

// ---- device side: ohreaction ------------------------------------------------------------------------------------------
#ifdef FPX_OH_HOST
// the level search of fpx_device.hpp (find_level), for the host build of oh_particle
template <typename R>
inline int find_level(const R *hgt, int nz, R zt) {
  int lo = 2, hi = nz;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (hgt[mid - 1] > zt) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}
FPX_OH_FN float oh_div(float a, float b) { return a / b; }
FPX_OH_FN double oh_div(double a, double b) { return a / b; }
#else
FPX_OH_FN float oh_div(float a, float b) { return __fdiv_rn(a, b); }
FPX_OH_FN double oh_div(double a, double b) { return __ddiv_rn(a, b); }
#endif
FPX_OH_FN float oh_pow(float a, float b) { return powf(a, b); }
FPX_OH_FN double oh_pow(double a, double b) { return pow(a, b); }
FPX_OH_FN float oh_exp(float a) { return expf(a); }
FPX_OH_FN double oh_exp(double a) { return exp(a); }
FPX_OH_FN float oh_abs(float a) { return fabsf(a); }
FPX_OH_FN double oh_abs(double a) { return fabs(a); }

template <typename H>
struct Args {
  int nxOH, nyOH, nzOH;
  int nztop;                      // nzOH - 1: the entries of altOHtop the search looks at (see oh_particle)
  const H *lon, *lat, *alttop;    // [nxOH], [nyOH], [nzOH]
  const H *oh;                    // the blended field, (ix,jy,kz) with ix fastest
  const H *d3;                    // (pv, qv, tt) of both slots of the mother grid, [jy][ix][iz][slot][3]
  int nx, ny, nz;
  int slot;                       // n - 1 of ohreaction.f90:85-87
  H dx, dy, xlon0, ylat0;
  int numbnests;
  H xl[kOhMaxNests], yl[kOhMaxNests], xr[kOhMaxNests], yr[kOhMaxNests], xres[kOhMaxNests], yres[kOhMaxNests];
  int nreact, spec[kOhMaxSpec];   // the species with ohcconst > 0, in order
  H cc[kOhMaxSpec], dc[kOhMaxSpec], nc[kOhMaxSpec];
  H tl;                           // abs(ltsample)
  H small;                        // tiny of the type xmass1 is kept in
  unsigned int *skipped;
};

// the discrete decisions of one particle (tests; the kernel drops them)
struct Pick { int ngrid, ix, jy, indz, ohx, ohy, ohz, reacted; };

// minloc(abs(a - x)) over a strictly increasing axis (check_axis), 0-based: the bracketing pair by bisection, then the
// reference's own differences on the two
template <typename H>
FPX_OH_FN int oh_nearest(const H *a, int n, H x) {
  FPX_OH_NOCONTRACT
  if (n < 2) return 0;
  int lo = 0, hi = n - 1;          // a[lo] <= x < a[hi] once x lies inside; the ends bracket everything else
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid; else hi = mid;
  }
  return oh_abs(a[hi] - x) < oh_abs(a[lo] - x) ? hi : lo;
}

// ohreaction.f90:63-151 for the particle at (xt, yt, zt): true if it takes part (oh_average > tiny), and then mass[k] of every
// reacting species k < A.nreact is replaced.  lon, lat, alttop, hgt: the axes and height where the caller staged them.
// status: 0 done, 1 position outside the mother grid (left untouched).
template <typename R, typename H>
FPX_OH_FN int oh_particle(const Args<H> &A, const H *lon, const H *lat, const H *alttop, const R *hgt, double xt, double yt, R zt,
                          R *mass, Pick *pick) {
  FPX_OH_NOCONTRACT
  if (!(xt > -2.e9 && xt < 2.e9 && yt > -2.e9 && yt < 2.e9)) return 1;
  int ngrid = 0;
  H nxl = (H)0, nyl = (H)0, nxres = (H)0, nyres = (H)0;
#pragma unroll
  for (int j = kOhMaxNests; j >= 1; j--)
    if (ngrid == 0 && j <= A.numbnests && xt > (double)A.xl[j - 1] && xt < (double)A.xr[j - 1] && yt > (double)A.yl[j - 1] && yt < (double)A.yr[j - 1]) {
      ngrid = j; nxl = A.xl[j - 1]; nyl = A.yl[j - 1]; nxres = A.xres[j - 1]; nyres = A.yres[j - 1];
    }
  int ix, jy;
  if (ngrid > 0) {
    const H xtn = (H)((xt - (double)nxl) * (double)nxres), ytn = (H)((yt - (double)nyl) * (double)nyres);
    ix = (int)xtn; jy = (int)ytn;
  } else { ix = (int)xt; jy = (int)yt; }
  if (ix < 0 || ix >= A.nx || jy < 0 || jy >= A.ny) return 1;
  const int indz = find_level(hgt, A.nz, zt);
  H xlon = (H)(xt * (double)A.dx + (double)A.xlon0);
  if (xlon > (H)180.) xlon = xlon - (H)360.;
  const H ylat = (H)(yt * (double)A.dy + (double)A.ylat0);
  const int ohx = oh_nearest(lon, A.nxOH, xlon), ohy = oh_nearest(lat, A.nyOH, ylat), ohz = oh_nearest(alttop, A.nztop, (H)zt);
  const H oh_average = A.oh[((size_t)ohz * A.nyOH + ohy) * A.nxOH + ohx];
  const bool react = oh_average > A.small;
  if (pick) { pick->ngrid = ngrid; pick->ix = ix; pick->jy = jy; pick->indz = indz; pick->ohx = ohx; pick->ohy = ohy; pick->ohz = ohz; pick->reacted = react; }
  if (!react) return 0;
  const H temp = A.d3[((((size_t)jy * A.nx + ix) * A.nz + (indz - 1)) * 2 + A.slot) * 3 + 2];
#pragma unroll
  for (int k = 0; k < kOhMaxSpec; k++)
    if (k < A.nreact) {
      const H ohrate = A.cc[k] * oh_pow(temp, A.nc[k]) * oh_exp(oh_div(-A.dc[k], temp)) * oh_average;
      const H restmass = (H)mass[k] * oh_exp((H)-1. * ohrate * A.tl);
      mass[k] = restmass > A.small ? (R)restmass : (R)0.;
    }
  return 0;
}

#ifndef FPX_OH_HOST
// oh(ix,jy,kz) = OH1 + (OH2-OH1)*(itime-memOHtime(1))/(memOHtime(2)-memOHtime(1)), ohreaction.f90:124-126; tnum and tden are the
// two differences, formed on the host in H
template <typename H>
__global__ void __launch_bounds__(256) k_oh_blend(const H *__restrict__ oh1, const H *__restrict__ oh2, H tnum, H tden, H *__restrict__ oh, long long n) {
  FPX_OH_NOCONTRACT
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const H a = oh1[i], b = oh2[i];
  oh[i] = a + oh_div((b - a) * tnum, tden);
}

// one lane per storage space; dynamic LDS: lonOH, latOH, altOHtop (H) and height (R)
template <typename R, typename H>
__global__ void __launch_bounds__(256) k_ohreaction(Args<H> A, Parts<R> P, const R *__restrict__ height, long long n) {
  FPX_OH_NOCONTRACT
  extern __shared__ __align__(8) unsigned char oh_lds[];
  H *lon = (H *)oh_lds, *lat = lon + A.nxOH, *top = lat + A.nyOH;
  R *hgt = (R *)(top + A.nzOH + ((A.nxOH + A.nyOH + A.nzOH) & 1));    // 8-byte aligned whatever H and R are
  for (int k = threadIdx.x; k < A.nxOH; k += blockDim.x) lon[k] = A.lon[k];
  for (int k = threadIdx.x; k < A.nyOH; k += blockDim.x) lat[k] = A.lat[k];
  for (int k = threadIdx.x; k < A.nzOH; k += blockDim.x) top[k] = A.alttop[k];
  for (int k = threadIdx.x; k < A.nz; k += blockDim.x) hgt[k] = height[k];
  __syncthreads();
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || P.itra1[s] == kOhDead) return;
  R mass[kOhMaxSpec];
#pragma unroll
  for (int k = 0; k < kOhMaxSpec; k++) mass[k] = k < A.nreact ? P.xmass1[(size_t)A.spec[k] * (size_t)P.cap + (size_t)s] : (R)0;
  R out[kOhMaxSpec];
#pragma unroll
  for (int k = 0; k < kOhMaxSpec; k++) out[k] = mass[k];
  const int st = oh_particle<R, H>(A, lon, lat, top, hgt, P.xt[s], P.yt[s], P.zt[s], out, nullptr);
  if (st == 1) { atomicAdd(A.skipped, 1u); return; }
#pragma unroll
  for (int k = 0; k < kOhMaxSpec; k++)
    if (k < A.nreact && !(out[k] == mass[k])) P.xmass1[(size_t)A.spec[k] * (size_t)P.cap + (size_t)s] = out[k];
}
#endif  // FPX_OH_HOST

}  // namespace oh
FPX_TU_CLOSE
}  // namespace fpx
