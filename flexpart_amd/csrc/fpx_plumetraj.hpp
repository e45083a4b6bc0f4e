// Plume trajectories and their clustering (iout = 4, 5): plumetraj.f90:56-230, which timemanager.f90:438 calls at an output
// time, with clustering.f90, centerofmass.f90, distance.f90, distance2.f90 and mean_mod's mean; run by fpx_plumetraj.
//
// The particles of every active release point are brought into one contiguous list in the order of their particle numbers
// (a stable radix sort of (release point, storage space) pairs laid out by particle number), which is the order the
// reference's loop meets them in: the seeds of the k-means are list entries, and every sum below has a fixed order.
// A list is cut into chunks of kChunk entries.  One block per chunk reduces the terms of its entries in a fixed order --
// per lane its kPer entries in turn, the lanes of a wave by a butterfly, the waves in turn -- into fp64 partials; a second
// small kernel adds the partials of a release point in chunk order, rounds once to the host's real kind H and applies the
// reference's formulas.  No float atomics: the results are bitwise the same from call to call, for any number of storage
// spaces and after a locality sort.
//   k_pt_key, k_pt_bounds    the list and where each release point's part of it begins
//   k_pt_seed                clustering.f90:58-72
//   k_pt_sweep / _seg        one pass of the loop :78-162, for the release points that have not left it yet
//   k_pt_final1 / _seg       plumetraj.f90:81-190 (po_gather, the flags, height above sea level), :172-180 of clustering,
//                            centerofmass, mean
//   k_pt_final2 / _seg       clustering.f90:185-190 and plumetraj.f90:208-213; the values of the record
// All arithmetic is in H with FMA contraction off, in the reference's order of operations; distance and distance2 keep
// their double internals.  What differs from the reference is the order of the sums and the library behind sin, cos, acos,
// atan2 (DESIGN section 21 bounds both).
// The per-particle terms, the per-release-point formulas and the formatter of the record compile as host code too
// (FPX_PT_HOST), for checks without a GPU.
#pragma once
#ifndef FPX_PT_HOST
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include "fpx_partavg.hpp"
#include <hip/hip_runtime.h>
#define FPX_PT_FN __device__ __forceinline__
#else
#include <cmath>
#define FPX_PT_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif
#include <cstdio>
#include <cstring>
#include <string>

namespace fpx {
FPX_TU_OPEN
namespace pt {

constexpr int kMaxCluster = 8;             // FPX_MAXCLUSTER
constexpr int kChunk = 1024;               // list entries per chunk: fixed, the sums depend on it
constexpr int kThreads = 256;
constexpr int kPer = kChunk / kThreads;
constexpr int kVals = 14 + 5 * kMaxCluster;
constexpr int kSweepQ = 5;                 // per cluster: count, sum of distance^2, x, y, z; then the total of distance^2
constexpr int kFinal1Q = 12;               // after the clusters' sums of height: see pt_final1_update
constexpr int kMaxQ = kSweepQ * kMaxCluster + 1;
constexpr int kMaxSweeps = 100;            // clustering.f90:78

#ifndef FPX_PT_HOST
FPX_PT_FN float pt_sin(float v) { return sinf(v); }
FPX_PT_FN double pt_sin(double v) { return sin(v); }
FPX_PT_FN float pt_cos(float v) { return cosf(v); }
FPX_PT_FN double pt_cos(double v) { return cos(v); }
FPX_PT_FN double pt_acos(double v) { return acos(v); }
FPX_PT_FN float pt_atan2(float a, float b) { return atan2f(a, b); }
FPX_PT_FN double pt_atan2(double a, double b) { return atan2(a, b); }
FPX_PT_FN float pt_sqrt(float v) { return __fsqrt_rn(v); }
FPX_PT_FN double pt_sqrt(double v) { return __dsqrt_rn(v); }
FPX_PT_FN float pt_div(float a, float b) { return __fdiv_rn(a, b); }
FPX_PT_FN double pt_div(double a, double b) { return __ddiv_rn(a, b); }
#else
inline float pt_sin(float v) { return sinf(v); }
inline double pt_sin(double v) { return sin(v); }
inline float pt_cos(float v) { return cosf(v); }
inline double pt_cos(double v) { return cos(v); }
inline double pt_acos(double v) { return acos(v); }
inline float pt_atan2(float a, float b) { return atan2f(a, b); }
inline double pt_atan2(double a, double b) { return atan2(a, b); }
inline float pt_sqrt(float v) { return sqrtf(v); }
inline double pt_sqrt(double v) { return sqrt(v); }
inline float pt_div(float a, float b) { return a / b; }
inline double pt_div(double a, double b) { return a / b; }
#endif
template <typename H> FPX_PT_FN H pt_abs(H v) { return v < (H)0 ? -v : v; }
// a literal of the default real kind: the decimal is rounded once, to H
template <typename H> FPX_PT_FN H pt_lit(float f, double d) { return sizeof(H) == 4 ? (H)f : (H)d; }
#define FPX_PT_LIT(H, x) pt_lit<H>(x##f, x)
template <typename H> FPX_PT_FN H pt_pi180() { return pt_div(FPX_PT_LIT(H, 3.14159265), (H)180.); }   // par_mod.f90:59-60

// One release point: where its particles lie in the list, the state of its k-means and its record.
template <typename H>
struct Seg {
  int begin, n;                            // list entries begin .. begin + n - 1
  int chunk0, nchunk;                      // its chunks
  int clustered;                           // n >= ncluster: clustering.f90:52
  int frozen;                              // has left the loop :78-162 (or never entered it)
  int iterations;                          // passes of the loop taken
  int numb[kMaxCluster];
  H xc[kMaxCluster], yc[kMaxCluster];      // xclust, yclust in radians
  H rmsclust[kMaxCluster], zclust[kMaxCluster];
  H rms, rmsold;
  H val[kVals];                            // the record from xcenter on (plumetraj.f90:218-225)
};

// xl(n)=xlon0+xtra1(i)*dx (plumetraj.f90:81-82): a double position with default reals, rounded on assignment
template <typename H>
FPX_PT_FN H pt_lonlat(H x0, H d, double t) {
#pragma clang fp contract(off)
  return (H)((double)x0 + t * (double)d);
}

// distance2.f90:43-56 with sin and cos of the two latitudes (of real(rlat, kind=dp)) supplied
template <typename H>
FPX_PT_FN H pt_distance2(H rlat1, H rlon1, double slat1, double clat1, H rlat2, H rlon2, double slat2, double clat2) {
#pragma clang fp contract(off)
  const H box = FPX_PT_LIT(H, 0.0003);
  if (pt_abs(rlat1 - rlat2) < box && pt_abs(rlon1 - rlon2) < box) return (H)0;
  const double cdlon = pt_cos((double)(rlon1 - rlon2));
  const double crd = slat1 * slat2 + clat1 * clat2 * cdlon;
  return (H)(6.3712e6 * pt_acos(crd) / 1000.0);
}

// distance.f90:43-54 (degrees) with sin and cos of the second latitude supplied
template <typename H>
FPX_PT_FN double pt_dpr() { return 180.0 / 3.14159265358979; }
template <typename H>
FPX_PT_FN H pt_distance(H rlat1, H rlon1, H rlat2, H rlon2, double slat2, double clat2) {
#pragma clang fp contract(off)
  const H box = FPX_PT_LIT(H, 0.03);
  if (pt_abs(rlat1 - rlat2) < box && pt_abs(rlon1 - rlon2) < box) return (H)0;
  const double dpr = pt_dpr<H>();
  const double clat1 = pt_cos((double)rlat1 / dpr), slat1 = pt_sin((double)rlat1 / dpr);
  const double cdlon = pt_cos((double)(rlon1 - rlon2) / dpr);
  const double crd = slat1 * slat2 + clat1 * clat2 * cdlon;
  return (H)(6.3712e6 * pt_acos(crd) / 1000.0);
}

// the centroids of one release point as a pass of the loop reads them
template <typename H>
struct Cent {
  H xc, yc;
  double s, c;                             // sin, cos of real(yclust, kind=dp)
};
template <typename H>
FPX_PT_FN void pt_cent(Cent<H> &t, H xc, H yc) {
  t.xc = xc; t.yc = yc;
  t.s = pt_sin((double)yc); t.c = pt_cos((double)yc);
}

// clustering.f90:85-95 and :113-131 for one particle at (xr, yr) radians: the nearest centroid (the first of equals; 0 when no
// distance compares, which the reference leaves to the previous particle's), the distance to it and the Cartesian terms
template <typename H>
FPX_PT_FN int pt_assign(int K, const Cent<H> *t, H xr, H yr, H &dmin, H &x, H &y, H &z) {
#pragma clang fp contract(off)
  const double slat1 = pt_sin((double)yr), clat1 = pt_cos((double)yr);
  H distancemin = (H)1.e10;                // 10.**10.
  int ncl = -1;
  for (int j = 0; j < K; j++) {
    const H d = pt_distance2<H>(yr, xr, slat1, clat1, t[j].yc, t[j].xc, t[j].s, t[j].c);
    if (d < distancemin) { distancemin = d; ncl = j; }
  }
  // :113: the same call again, the same value
  if (ncl >= 0) dmin = distancemin;
  else { ncl = 0; dmin = pt_distance2<H>(yr, xr, slat1, clat1, t[0].yc, t[0].xc, t[0].s, t[0].c); }
  const H cy = sizeof(H) == 8 ? (H)clat1 : pt_cos(yr), sy = sizeof(H) == 8 ? (H)slat1 : pt_sin(yr);
  x = cy * pt_sin(xr);
  y = (H)-1. * cy * pt_cos(xr);
  z = sy;
  return ncl;
}

// centerofmass.f90:35-43 for one particle at (xl, yl) degrees
template <typename H>
FPX_PT_FN void pt_cart(H xl, H yl, H &x, H &y, H &z) {
#pragma clang fp contract(off)
  const H pi180 = pt_pi180<H>();
  const H xll = xl * pi180, yll = yl * pi180;
  const H cy = pt_cos(yll);
  x = cy * pt_sin(xll);
  y = (H)-1. * cy * pt_cos(xll);
  z = pt_sin(yll);
}

// what clustering leaves in xl, yl (:58-62, :169-171) when it runs at all
template <typename H>
FPX_PT_FN H pt_roundtrip(H v, int clustered) {
#pragma clang fp contract(off)
  const H pi180 = pt_pi180<H>();
  return clustered ? pt_div(v * pi180, pi180) : v;
}

// plumetraj.f90:143-147, :169, :171: bit 0 within the PBL, bit 1 |PV| < 2 pvu on the hemisphere's side, bit 2 below the tropopause
template <typename H>
FPX_PT_FN int pt_flags(H yl, H zl, H pvi, H tri, H hmixi) {
  int f = 0;
  if (yl > (H)0.) { if (pvi < (H)2.) f |= 2; } else { if (pvi > (H)-2.) f |= 2; }
  if (zl < tri) f |= 4;
  if (zl < hmixi) f |= 1;
  return f;
}

// clustering.f90:134-160 from the sums of pass l (s[5 j + 0..4]: numb, sum of distances^2, xav, yav, zav of cluster j;
// s[5 K]: the sum of all distances^2); true when the loop is left
template <typename H>
FPX_PT_FN bool pt_sweep_update(Seg<H> &S, int K, const double *s, int l) {
#pragma clang fp contract(off)
  const H rms = pt_sqrt(pt_div((H)s[kSweepQ * K], (H)S.n));
  for (int j = 0; j < K; j++) {
    const int numb = (int)s[kSweepQ * j];
    S.numb[j] = numb;
    S.rmsclust[j] = (H)0;
    if (numb > 0) {
      const H nb = (H)numb;
      S.rmsclust[j] = pt_sqrt(pt_div((H)s[kSweepQ * j + 1], nb));
      const H xav = pt_div((H)s[kSweepQ * j + 2], nb), yav = pt_div((H)s[kSweepQ * j + 3], nb), zav = pt_div((H)s[kSweepQ * j + 4], nb);
      S.xc[j] = pt_atan2(xav, (H)-1. * yav);
      S.yc[j] = pt_atan2(zav, pt_sqrt(xav * xav + yav * yav));
    }
  }
  S.rms = rms;
  S.iterations = l;
  if (l > 1 && pt_div(pt_abs(rms - S.rmsold), S.rmsold) < FPX_PT_LIT(H, 0.005)) return true;
  S.rmsold = rms;
  return false;
}

// plumetraj.f90:184-190, clustering.f90:172-180 (zclust), centerofmass.f90:54-69, mean_mod's mean from the sums
// s[0..K-1]: the heights above sea level by cluster; then topo, hmixi, pvi, tri and topo; the counts within the PBL, of |PV| < 2
// and below the tropopause; the Cartesian x, y, z of centerofmass; the heights and their squares
template <typename H>
FPX_PT_FN void pt_final1_update(Seg<H> &S, int K, const double *s) {
#pragma clang fp contract(off)
  const H n = (H)S.n, pi180 = pt_pi180<H>();
  const double *t = s + K;
  S.val[3] = pt_div((H)t[0], n);
  S.val[4] = pt_div((H)t[1], n);
  S.val[6] = pt_div((H)t[2], n);
  S.val[5] = pt_div((H)t[3], n);
  S.val[11] = pt_div((H)100. * (H)t[4], n);
  S.val[12] = pt_div((H)100. * (H)t[5], n);
  S.val[13] = pt_div((H)100. * (H)t[6], n);
  for (int j = 0; j < K; j++) S.zclust[j] = S.clustered && S.numb[j] > 0 ? pt_div((H)s[j], (H)S.numb[j]) : (H)0;
  const H xav = pt_div((H)t[7], n), yav = pt_div((H)t[8], n), zav = pt_div((H)t[9], n);
  S.val[0] = pt_div(pt_atan2(xav, (H)-1. * yav), pi180);
  S.val[1] = pt_div(pt_atan2(zav, pt_sqrt(xav * xav + yav * yav)), pi180);
  const H xl = (H)t[10], xq = (H)t[11];
  S.val[2] = pt_div(xl, n);
  const H xaux = xq - pt_div(xl * xl, n);
  S.val[9] = xaux < FPX_PT_LIT(H, 1.0e-30) ? (H)0 : pt_sqrt(pt_div(xaux, (H)(S.n - 1)));
}

// clustering.f90:175-190 and plumetraj.f90:212-213 from s[0]: the sum of (zl - zclust)^2, s[1]: the sum of distance^2 from
// the centre; completes the record.  A release point with fewer particles than clusters: zeros where the reference prints
// what its locals happened to hold.
template <typename H>
FPX_PT_FN void pt_final2_update(Seg<H> &S, int K, const double *s) {
#pragma clang fp contract(off)
  const H n = (H)S.n, pi180 = pt_pi180<H>();
  H rmsdist = (H)s[1];
  if (rmsdist > (H)0.) rmsdist = pt_sqrt(pt_div(rmsdist, n));
  S.val[7] = rmsdist > (H)0. ? rmsdist : (H)0.;
  H zrms = (H)0;
  if (S.clustered) {
    zrms = (H)s[0];
    if (zrms > (H)0.) zrms = pt_sqrt(pt_div(zrms, n));
  }
  S.val[8] = S.clustered ? S.rms : (H)0;
  S.val[10] = zrms;
  for (int j = 0; j < K; j++) {
    H *c = S.val + 14 + 5 * j;
    if (S.clustered) {
      c[0] = pt_div(S.xc[j], pi180);
      c[1] = pt_div(S.yc[j], pi180);
      c[2] = S.zclust[j];
      c[3] = pt_div((H)100. * (H)S.numb[j], n);
      c[4] = S.rmsclust[j];
    } else {
      c[0] = c[1] = c[2] = c[3] = c[4] = (H)0;
    }
  }
}

// ---- the formatter (host) ----------------------------------------------------------------------------------------------
// Fw.d as the reference's runtime writes it: the exact binary value rounded to d places, ties to even; the optional zero
// before the point dropped when the field is too narrow for it; asterisks when it still does not fit.
inline void pt_put_f(std::string &out, double v, int w, int d) {
  char b[512];
  if (v != v) snprintf(b, sizeof b, "NaN");
  else if (v - v != 0.) snprintf(b, sizeof b, v < 0 ? "-Inf" : "Inf");
  else if (d == 0) snprintf(b, sizeof b, "%#.0f", v);
  else snprintf(b, sizeof b, "%.*f", d, v);
  std::string t = b;
  if ((int)t.size() > w) {
    const size_t z = t[0] == '-' ? 1 : 0;
    if (t.size() > z + 1 && t[z] == '0' && t[z + 1] == '.') t.erase(z, 1);
  }
  if ((int)t.size() > w) t.assign((size_t)w, '*');
  out.append((size_t)w - t.size(), ' ');
  out += t;
}
inline void pt_put_i(std::string &out, long long v, int w) {
  char b[32];
  snprintf(b, sizeof b, "%lld", v);
  std::string t = b;
  if ((int)t.size() > w) t.assign((size_t)w, '*');
  out.append((size_t)w - t.size(), ' ');
  out += t;
}
// (i5,i8,2f9.4,4f8.1,f8.2,4f8.1,3f6.1,5(2f8.3,f7.0,f6.1,f8.1)), plumetraj.f90:218-225, with its newline
template <typename H>
inline std::string pt_record(int j, int age, const H *val) {
  static const int w[14] = {9, 9, 8, 8, 8, 8, 8, 8, 8, 8, 8, 6, 6, 6}, d[14] = {4, 4, 1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1};
  static const int wc[5] = {8, 8, 7, 6, 8}, dc[5] = {3, 3, 0, 1, 1};
  std::string s;
  pt_put_i(s, j, 5);
  pt_put_i(s, age, 8);
  for (int k = 0; k < 14; k++) pt_put_f(s, (double)val[k], w[k], d[k]);
  for (int c = 0; c < 5; c++)
    for (int k = 0; k < 5; k++) pt_put_f(s, (double)val[14 + 5 * c + k], wc[k], dc[k]);
  s += '\n';
  return s;
}

#ifndef FPX_PT_HOST
// ---- kernels -----------------------------------------------------------------------------------------------------------
// key[pid] = npoint - 1 for a member of an active release point (plumetraj.f90:65,78-79), numpoint for everything else;
// val[pid] = the storage space.  Not a member either: a position outside the met grid or not finite (the reference would
// index its fields out of bounds).
template <typename R>
__global__ void __launch_bounds__(256) k_pt_key(View<R> V, Parts<R> P, long long numpart, int itime, int numpoint,
                                                const unsigned char *__restrict__ active, unsigned int *__restrict__ key,
                                                unsigned int *__restrict__ val) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart) return;
  const unsigned int pid = P.pid[s];
  if ((long long)pid >= numpart) return;   // cannot happen: the particle numbers of the storage spaces in use are a permutation
  unsigned int k = (unsigned int)numpoint;
  const int np = P.npoint[s];
  if (P.itra1[s] == itime && np >= 1 && np <= numpoint && active[np - 1]) {
    const double xt = P.xt[s], yt = P.yt[s];
    const R zt = P.zt[s];
    if (xt >= 0. && xt < (double)(R)V.nxmin1 && yt >= 0. && yt <= (double)(R)V.nymin1 && zt - zt == (R)0) k = (unsigned int)(np - 1);
  }
  key[pid] = k;
  val[pid] = (unsigned int)s;
}

// start[k] = the first list entry whose key is >= k, k = 0 .. numpoint
__global__ void __launch_bounds__(256) k_pt_bounds(const unsigned int *__restrict__ key, long long n, int numpoint, int *__restrict__ start) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > numpoint) return;
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (key[mid] < (unsigned int)k) lo = mid + 1; else hi = mid;
  }
  start[k] = (int)lo;
}

template <typename H>
struct Geo { H xlon0, ylat0, dx, dy; };

// clustering.f90:68-72: the seeds are list entries j*n/ncluster, j = 1 .. ncluster
template <typename R, typename H>
__global__ void __launch_bounds__(64) k_pt_seed(Parts<R> P, Geo<H> G, Seg<H> *__restrict__ segs, int numpoint, int K,
                                                const unsigned int *__restrict__ list) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numpoint * K) return;
  Seg<H> &S = segs[i / K];
  const int j = i % K;
  if (!S.clustered) return;
  const long long e = (long long)S.begin + (long long)(j + 1) * S.n / K - 1;
  const unsigned int s = list[e];
  const H pi180 = pt_pi180<H>();
  S.xc[j] = pt_lonlat<H>(G.xlon0, G.dx, P.xt[s]) * pi180;
  S.yc[j] = pt_lonlat<H>(G.ylat0, G.dy, P.yt[s]) * pi180;
  if (j == 0) S.rmsold = (H)-5.;
}

// v[0 .. NQ-1] of every lane of the block -> out[0 .. NQ-1], in a fixed order: the lanes of a wave by a butterfly (every
// lane ends with the same bits, a + b = b + a), then the waves in turn
template <int NQ>
__device__ __forceinline__ void pt_block_sum(double (&v)[NQ], double *__restrict__ out, double (*lds)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; q++)
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NQ; q++) lds[wave][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    double a = lds[0][threadIdx.x];
    for (int w = 1; w < kThreads / 64; w++) a += lds[w][threadIdx.x];
    out[threadIdx.x] = a;
  }
}

// One pass of clustering.f90:85-132 over one chunk.  xl, yl are formed again from the position (plumetraj.f90:81-82,
// clustering.f90:60-61).  ncl: the particle's cluster, one byte per list entry; part: [chunk][kMaxQ].
template <typename R, typename H, int KM>
__global__ void __launch_bounds__(kThreads) k_pt_sweep(Parts<R> P, Geo<H> G, const Seg<H> *__restrict__ segs, const int *__restrict__ chunk_seg,
                                                       const unsigned int *__restrict__ list, unsigned char *__restrict__ ncl,
                                                       double *__restrict__ part, int K) {
#pragma clang fp contract(off)
  __shared__ Cent<H> cent[KM];
  __shared__ double lds[kThreads / 64][kSweepQ * KM + 1];
  const int c = blockIdx.x;
  const Seg<H> &S = segs[chunk_seg[c]];
  if (S.frozen) return;                    // the whole block
  if (threadIdx.x < K) pt_cent<H>(cent[threadIdx.x], S.xc[threadIdx.x], S.yc[threadIdx.x]);
  __syncthreads();
  const int first = (c - S.chunk0) * kChunk, count = min(kChunk, S.n - first);
  const H pi180 = pt_pi180<H>();
  double v[kSweepQ * KM + 1];
#pragma unroll
  for (int q = 0; q < kSweepQ * KM + 1; q++) v[q] = 0.;
  for (int i = 0; i < kPer; i++) {
    const int k = threadIdx.x + i * kThreads;
    if (k >= count) break;
    const long long e = (long long)S.begin + first + k;
    const unsigned int s = list[e];
    const H xr = pt_lonlat<H>(G.xlon0, G.dx, P.xt[s]) * pi180, yr = pt_lonlat<H>(G.ylat0, G.dy, P.yt[s]) * pi180;
    H d, x, y, z;
    const int m = pt_assign<H>(K, cent, xr, yr, d, x, y, z);
    ncl[e] = (unsigned char)m;
    const double d2 = (double)(d * d);
#pragma unroll
    for (int j = 0; j < KM; j++) {
      const bool mine = j == m;
      v[kSweepQ * j] += mine ? 1. : 0.;
      v[kSweepQ * j + 1] += mine ? d2 : 0.;
      v[kSweepQ * j + 2] += mine ? (double)x : 0.;
      v[kSweepQ * j + 3] += mine ? (double)y : 0.;
      v[kSweepQ * j + 4] += mine ? (double)z : 0.;
    }
    v[kSweepQ * KM] += d2;
  }
  pt_block_sum<kSweepQ * KM + 1>(v, part + (size_t)c * kMaxQ, lds);
}

// the partials of a release point in chunk order -> tot[0 .. nq-1].  Sixteen loads are in flight before their sixteen
// additions, which keep the order: one lane adds the 1e4 chunks of a 1e7-particle point, and a load per addition would
// cost a round trip to memory each (measured: 1.6 ms per call of this function instead of 0.1).
__device__ __forceinline__ void pt_seg_sum(const double *__restrict__ part, int chunk0, int nchunk, int nq, double *tot) {
  if ((int)threadIdx.x < nq) {
    const double *p = part + (size_t)chunk0 * kMaxQ + threadIdx.x;
    double a = 0.;
    int c = 0;
    for (; c + 16 <= nchunk; c += 16) {
      double t[16];
#pragma unroll
      for (int k = 0; k < 16; k++) t[k] = p[(size_t)(c + k) * kMaxQ];
#pragma unroll
      for (int k = 0; k < 16; k++) a += t[k];
    }
    for (; c < nchunk; c++) a += p[(size_t)c * kMaxQ];
    tot[threadIdx.x] = a;
  }
  __syncthreads();
}

// clustering.f90:134-160 per release point; pending[l]: some release point goes on
template <typename H, int KM>
__global__ void __launch_bounds__(64) k_pt_sweep_seg(Seg<H> *__restrict__ segs, const double *__restrict__ part, int K, int l, int *__restrict__ pending) {
  __shared__ double tot[kMaxQ];
  Seg<H> &S = segs[blockIdx.x];
  if (S.frozen) return;
  pt_seg_sum(part, S.chunk0, S.nchunk, kSweepQ * KM + 1, tot);
  if (threadIdx.x != 0) return;
  double s[kMaxQ];
  for (int j = 0; j < K; j++)
    for (int q = 0; q < kSweepQ; q++) s[kSweepQ * j + q] = tot[kSweepQ * j + q];
  s[kSweepQ * K] = tot[kSweepQ * KM];
  if (pt_sweep_update<H>(S, K, s, l) || l >= kMaxSweeps) S.frozen = 1;
  else pending[l] = 1;
}

// plumetraj.f90:83-173 per particle, the sums of zclust (clustering.f90:172), centerofmass and mean.  zl: the height above
// sea level, one H per list entry.
template <typename R, typename H, int KM>
__global__ void __launch_bounds__(kThreads) k_pt_final1(View<R> V, Parts<R> P, DiagP<H> D, const Seg<H> *__restrict__ segs,
                                                        const int *__restrict__ chunk_seg, const unsigned int *__restrict__ list,
                                                        const unsigned char *__restrict__ ncl, H *__restrict__ zl, double *__restrict__ part, int itime) {
#pragma clang fp contract(off)
  __shared__ double lds[kThreads / 64][KM + kFinal1Q];
  const int c = blockIdx.x;
  const Seg<H> &S = segs[chunk_seg[c]];
  const int first = (c - S.chunk0) * kChunk, count = min(kChunk, S.n - first);
  const int clustered = S.clustered;
  double v[KM + kFinal1Q];
#pragma unroll
  for (int q = 0; q < KM + kFinal1Q; q++) v[q] = 0.;
  for (int i = 0; i < kPer; i++) {
    const int k = threadIdx.x + i * kThreads;
    if (k >= count) break;
    const long long e = (long long)S.begin + first + k;
    const unsigned int s = list[e];
    const H zt = (H)P.zt[s];
    PoVals<H> o;
    po_gather<R, H, false>(V, D, itime, P.xt[s], P.yt[s], zt, o);
    const int f = pt_flags<H>(o.ylat, zt, o.pvi, o.tri, o.hmixi);
    const H z = zt + o.topo;
    zl[e] = z;
    const int m = clustered ? (int)ncl[e] : -1;
#pragma unroll
    for (int j = 0; j < KM; j++) v[j] += j == m ? (double)z : 0.;
    H x, y, zc;
    pt_cart<H>(pt_roundtrip<H>(o.xlon, clustered), pt_roundtrip<H>(o.ylat, clustered), x, y, zc);
    v[KM + 0] += (double)o.topo;
    v[KM + 1] += (double)o.hmixi;
    v[KM + 2] += (double)o.pvi;
    v[KM + 3] += (double)o.tri + (double)o.topo;   // tropocenter=tropocenter+tri+topo adds them one after the other
    v[KM + 4] += (f & 1) ? 1. : 0.;
    v[KM + 5] += (f & 2) ? 1. : 0.;
    v[KM + 6] += (f & 4) ? 1. : 0.;
    v[KM + 7] += (double)x;
    v[KM + 8] += (double)y;
    v[KM + 9] += (double)zc;
    v[KM + 10] += (double)z;
    v[KM + 11] += (double)(z * z);
  }
  pt_block_sum<KM + kFinal1Q>(v, part + (size_t)c * kMaxQ, lds);
}

template <typename H, int KM>
__global__ void __launch_bounds__(64) k_pt_final1_seg(Seg<H> *__restrict__ segs, const double *__restrict__ part, int K) {
  __shared__ double tot[kMaxQ];
  Seg<H> &S = segs[blockIdx.x];
  if (S.n <= 0) return;
  pt_seg_sum(part, S.chunk0, S.nchunk, KM + kFinal1Q, tot);
  if (threadIdx.x != 0) return;
  double s[kMaxQ];
  for (int j = 0; j < K; j++) s[j] = tot[j];
  for (int q = 0; q < kFinal1Q; q++) s[K + q] = tot[KM + q];
  pt_final1_update<H>(S, K, s);
}

// clustering.f90:186-189 and plumetraj.f90:208-211 per particle
template <typename R, typename H>
__global__ void __launch_bounds__(kThreads) k_pt_final2(Parts<R> P, Geo<H> G, const Seg<H> *__restrict__ segs, const int *__restrict__ chunk_seg,
                                                        const unsigned int *__restrict__ list, const unsigned char *__restrict__ ncl,
                                                        const H *__restrict__ zl, double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double lds[kThreads / 64][2];
  const int c = blockIdx.x;
  const Seg<H> &S = segs[chunk_seg[c]];
  const int first = (c - S.chunk0) * kChunk, count = min(kChunk, S.n - first);
  const int clustered = S.clustered;
  const H xcenter = S.val[0], ycenter = S.val[1];
  const double dpr = pt_dpr<H>();
  const double slat2 = pt_sin((double)ycenter / dpr), clat2 = pt_cos((double)ycenter / dpr);
  double v[2] = {0., 0.};
  for (int i = 0; i < kPer; i++) {
    const int k = threadIdx.x + i * kThreads;
    if (k >= count) break;
    const long long e = (long long)S.begin + first + k;
    const unsigned int s = list[e];
    if (clustered) {
      const H zdist = zl[e] - S.zclust[ncl[e]];
      v[0] += (double)(zdist * zdist);
    }
    const H xl = pt_roundtrip<H>(pt_lonlat<H>(G.xlon0, G.dx, P.xt[s]), clustered), yl = pt_roundtrip<H>(pt_lonlat<H>(G.ylat0, G.dy, P.yt[s]), clustered);
    const H dist = pt_distance<H>(yl, xl, ycenter, xcenter, slat2, clat2);
    v[1] += (double)(dist * dist);
  }
  pt_block_sum<2>(v, part + (size_t)c * kMaxQ, lds);
}

template <typename H>
__global__ void __launch_bounds__(64) k_pt_final2_seg(Seg<H> *__restrict__ segs, const double *__restrict__ part, int K) {
  __shared__ double tot[kMaxQ];
  Seg<H> &S = segs[blockIdx.x];
  if (S.n <= 0) return;
  pt_seg_sum(part, S.chunk0, S.nchunk, 2, tot);
  if (threadIdx.x != 0) return;
  const double s[2] = {tot[0], tot[1]};
  pt_final2_update<H>(S, K, s);
}
#endif

}  // namespace pt
FPX_TU_CLOSE
}  // namespace fpx
