// Per-particle averages over the output interval (ipout = 3; fpx_config.device_partavg): partpos_average.f90:31-184, which
// the particle loop calls after advance (timemanager.f90:617), and partoutput_average.f90:54-201 (timemanager.f90:455).
//
// po_gather is the interpolation to the particle's position that partoutput.f90:63-175 and partpos_average.f90:31-152 share
// word for word -- topography, PV, humidity, temperature, density, tropopause, mixing height, and for the averages the two
// wind components -- in the host's real kind H, in the reference's order, FMA contraction off; k_partoutput (fpx_particles.hpp)
// and k_partavg both call it.  Where the reference mixes kinds (xlon, ddx, ddy: a double position with default reals) the
// expression is formed in double and rounded to H.  uu and vv come from the unblended wind pack of the two time slots
// whether or not the step's blended pack exists: the blended pack rounds in another order.
// k_partavg runs after the kernels that move the particle, one lane per storage space: a space that was due in this step adds
// its values to fourteen running sums and counts the call; k_partavg_out turns the sums into the twelve int16 of a record of
// partposit_average_*, at the record of the particle's number, and zeroes the fifteen values of every space.
// The sums are SoA over the storage spaces like Parts; k_partavg_permute moves them with the particle in a locality sort.
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>

namespace fpx {
FPX_TU_OPEN

template <typename H>
struct DiagP {
  const H *oro, *tropo[2];   // host layout (ix,jy), stride nxmax
  const H *d3;               // [jy][ix][iz][slot][3] = (pv, qv, tt): z fastest like the wind pack, one 96-byte run per corner column
  int nxmax, nymax;
  H dx, dy, xlon0, ylat0;
};

template <typename H>
struct PoVals {
  H xlon, ylat, topo, pvi, qvi, tti, rhoi, hmixi, tri, uui, vvi;
};

// partoutput.f90:69-175 = partpos_average.f90:31-152 for a particle at (xt, yt, zt).  The caller has made sure that
// 0 <= xt < nx - 1 and 0 <= yt <= ny - 1.  WIND: also uu, vv (partpos_average.f90:103-111,121-122,128-129).
template <typename R, typename H, bool WIND>
__device__ __forceinline__ void po_gather(const View<R> &V, const DiagP<H> &D, int itime, double xt, double yt, H zt, PoVals<H> &o) {
#pragma clang fp contract(off)
  const int nx = V.nx, ny = V.ny, nz = V.nz;
  const H dt1 = (H)(itime - V.memtime0), dt2 = (H)(V.memtime1 - itime);   // partoutput.f90:69-71
  const H dtt = (H)1. / (dt1 + dt2);
  o.xlon = (H)((double)D.xlon0 + xt * (double)D.dx);
  o.ylat = (H)((double)D.ylat0 + yt * (double)D.dy);
  const int ix = (int)xt, jy = (int)yt;
  int ixp = ix + 1, jyp = jy + 1;
  const H ddx = (H)(xt - (double)(H)ix), ddy = (H)(yt - (double)(H)jy);
  const H rddx = (H)1. - ddx, rddy = (H)1. - ddy;
  const H p1 = rddx * rddy, p2 = ddx * rddy, p3 = rddx * ddy, p4 = ddx * ddy;
  if (jyp >= D.nymax) jyp = jyp - 1;                                      // :119-121
  if (ixp >= D.nxmax) ixp = D.nxmax - 1;                                  // guard (weight 0 there)
  auto h2 = [&](const H *f, int i, int j) { return f[(size_t)i + (size_t)D.nxmax * (size_t)j]; };
  // component c of (pv, qv, tt) at level k, slot h; elements of the host's padding read as 0 like rho below
  auto d3 = [&](int c, int i, int j, int k, int h) -> H {
    if (i >= nx || j >= ny) return (H)0;
    return D.d3[((((size_t)j * nx + i) * nz + (k - 1)) * 2 + h) * 3 + c];
  };
  // rho, hmix and the winds live in the gather packs (compact nx, ny; elements of the host's padding read as 0)
  auto rho_at = [&](int i, int j, int k, int slot) -> H {
    if (i >= nx || j >= ny) return (H)0;
    return (H)V.r2[(((size_t)j * nx + i) * nz + (k - 1)) * 4 + slot * 2];
  };
  auto hmix_at = [&](int i, int j, int slot) -> H {
    if (i >= nx || j >= ny) return (H)0;
    return (H)V.sfc[((size_t)j * nx + i) * 8 + slot * 4 + 3];
  };
  auto w_at = [&](int c, int i, int j, int k, int slot) -> H {
    if (i >= nx || j >= ny) return (H)0;
    return (H)V.w3[((((size_t)j * nx + i) * nz + (k - 1)) * 2 + slot) * 3 + c];
  };
  o.topo = p1 * h2(D.oro, ix, jy) + p2 * h2(D.oro, ixp, jy) + p3 * h2(D.oro, ix, jyp) + p4 * h2(D.oro, ixp, jyp);
  int indz = nz - 1, indzp = nz;   // the reference keeps the previous particle's indices when zt >= height(nz); cannot happen after advance()
  for (int il = 2; il <= nz; il++)
    if ((H)V.height[il - 1] > zt) { indz = il - 1; indzp = il; break; }
  const H dz1 = zt - (H)V.height[indz - 1], dz2 = (H)V.height[indzp - 1] - zt;
  const H dz = (H)1. / (dz1 + dz2);
  const int slot[2] = {V.m1, V.m2};
  H pvprof[2], qvprof[2], ttprof[2], rhoprof[2], uuprof[2], vvprof[2];
#pragma unroll
  for (int l = 0; l < 2; l++) {
    const int ind = indz + l;
    H pv1[2], qv1[2], tt1[2], rho1[2], uu1[2], vv1[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const int h = slot[m];
      pv1[m] = p1 * d3(0, ix, jy, ind, h) + p2 * d3(0, ixp, jy, ind, h) + p3 * d3(0, ix, jyp, ind, h) + p4 * d3(0, ixp, jyp, ind, h);
      qv1[m] = p1 * d3(1, ix, jy, ind, h) + p2 * d3(1, ixp, jy, ind, h) + p3 * d3(1, ix, jyp, ind, h) + p4 * d3(1, ixp, jyp, ind, h);
      tt1[m] = p1 * d3(2, ix, jy, ind, h) + p2 * d3(2, ixp, jy, ind, h) + p3 * d3(2, ix, jyp, ind, h) + p4 * d3(2, ixp, jyp, ind, h);
      if (WIND) {
        uu1[m] = p1 * w_at(0, ix, jy, ind, h) + p2 * w_at(0, ixp, jy, ind, h) + p3 * w_at(0, ix, jyp, ind, h) + p4 * w_at(0, ixp, jyp, ind, h);
        vv1[m] = p1 * w_at(1, ix, jy, ind, h) + p2 * w_at(1, ixp, jy, ind, h) + p3 * w_at(1, ix, jyp, ind, h) + p4 * w_at(1, ixp, jyp, ind, h);
      }
      rho1[m] = p1 * rho_at(ix, jy, ind, h) + p2 * rho_at(ixp, jy, ind, h) + p3 * rho_at(ix, jyp, ind, h) + p4 * rho_at(ixp, jyp, ind, h);
    }
    pvprof[l] = (pv1[0] * dt2 + pv1[1] * dt1) * dtt;
    qvprof[l] = (qv1[0] * dt2 + qv1[1] * dt1) * dtt;
    ttprof[l] = (tt1[0] * dt2 + tt1[1] * dt1) * dtt;
    if (WIND) {
      uuprof[l] = (uu1[0] * dt2 + uu1[1] * dt1) * dtt;
      vvprof[l] = (vv1[0] * dt2 + vv1[1] * dt1) * dtt;
    }
    rhoprof[l] = (rho1[0] * dt2 + rho1[1] * dt1) * dtt;
  }
  o.pvi = (dz1 * pvprof[1] + dz2 * pvprof[0]) * dz;
  o.qvi = (dz1 * qvprof[1] + dz2 * qvprof[0]) * dz;
  o.tti = (dz1 * ttprof[1] + dz2 * ttprof[0]) * dz;
  if (WIND) {
    o.uui = (dz1 * uuprof[1] + dz2 * uuprof[0]) * dz;
    o.vvi = (dz1 * vvprof[1] + dz2 * vvprof[0]) * dz;
  } else {
    o.uui = (H)0; o.vvi = (H)0;
  }
  o.rhoi = (dz1 * rhoprof[1] + dz2 * rhoprof[0]) * dz;
  H tr[2], hm[2];
#pragma unroll
  for (int m = 0; m < 2; m++) {
    const int h = slot[m];
    tr[m] = p1 * h2(D.tropo[h], ix, jy) + p2 * h2(D.tropo[h], ixp, jy) + p3 * h2(D.tropo[h], ix, jyp) + p4 * h2(D.tropo[h], ixp, jyp);
    hm[m] = p1 * hmix_at(ix, jy, h) + p2 * hmix_at(ixp, jy, h) + p3 * hmix_at(ix, jyp, h) + p4 * hmix_at(ixp, jyp, h);
  }
  o.hmixi = (hm[0] * dt2 + hm[1] * dt1) * dtt;
  o.tri = (tr[0] * dt2 + tr[1] * dt1) * dtt;
}

namespace pa {

constexpr int kSums = 14;
// order of the sums (com_mod.f90:688-691 as fpx_get_partavg returns them)
enum { CARTX = 0, CARTY, CARTZ, Z, TOPO, PV, QV, TT, UU, VV, RHO, TRO, HMIX, ENERGY };

template <typename H>
struct State {
  int *npart_av;     // [cap]
  H *sum;            // [kSums][cap]
  long long cap;
};

__device__ __forceinline__ float pa_sin(float v) { return sinf(v); }
__device__ __forceinline__ double pa_sin(double v) { return sin(v); }
__device__ __forceinline__ float pa_cos(float v) { return cosf(v); }
__device__ __forceinline__ double pa_cos(double v) { return cos(v); }
__device__ __forceinline__ float pa_atan2(float a, float b) { return atan2f(a, b); }
__device__ __forceinline__ double pa_atan2(double a, double b) { return atan2(a, b); }
__device__ __forceinline__ float pa_sqrt(float v) { return __fsqrt_rn(v); }
__device__ __forceinline__ double pa_sqrt(double v) { return __dsqrt_rn(v); }
__device__ __forceinline__ float pa_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double pa_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float pa_round(float v) { return roundf(v); }
__device__ __forceinline__ double pa_round(double v) { return round(v); }

// timemanager.f90:617 for every storage space that was due in this step (notdue: the key k_prep gave the others).  The
// position is the one advance left.  A particle that advance stopped (nstop = 3: outside the grid, or not finite; the
// epilogue has terminated it) or that k_prep found outside is skipped: the reference would index the fields out of bounds.
template <typename R, typename H>
__global__ void __launch_bounds__(256) k_partavg(View<R> V, Parts<R> P, DiagP<H> D, State<H> S, const unsigned char *__restrict__ key,
                                                 unsigned char notdue, long long n, int itime) {
#pragma clang fp contract(off)
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || key[s] == notdue) return;
  const double xt = P.xt[s], yt = P.yt[s];
  const H zt = (H)P.zt[s];
  if (!(xt >= 0.) || !(xt < (double)(R)V.nxmin1) || !(yt >= 0.) || !(yt <= (double)(R)V.nymin1) || !(zt - zt == (H)0)) return;
  PoVals<H> o;
  po_gather<R, H, true>(V, D, itime, xt, yt, zt, o);
  const H cpa = (H)1004.6, pi180 = pa_div((H)3.14159265, (H)180.);      // par_mod.f90:61-63
  const H energy = o.tti * cpa + (zt + o.topo) * (H)9.81 + o.qvi * (H)2501000. + pa_div(o.uui * o.uui + o.vvi * o.vvi, (H)2.);   // :155
  const H xlon = o.xlon * pi180, ylat = o.ylat * pi180;                  // :165-169
  const H cy = pa_cos(ylat);
  const H x = cy * pa_sin(xlon);
  const H y = (H)-1. * cy * pa_cos(xlon);
  const H z = pa_sin(ylat);
  S.npart_av[s] = S.npart_av[s] + 1;
  const H add[kSums] = {x, y, z, zt, o.topo, o.pvi, o.qvi, o.tti, o.uui, o.vvi, o.rhoi, o.tri, o.hmixi, energy};
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    H *p = S.sum + (size_t)k * (size_t)S.cap + (size_t)s;
    *p = *p + add[k];
  }
}

// the sums follow their particle: B[i] = A[perm[i]] for the n spaces the sort permutes, B[i] = A[i] beyond
template <typename H>
__global__ void __launch_bounds__(256) k_partavg_permute(State<H> A, State<H> B, const unsigned int *__restrict__ perm, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.cap) return;
  const long long j = i < n ? (long long)perm[i] : i;
  B.npart_av[i] = A.npart_av[j];
#pragma unroll
  for (int k = 0; k < kSums; k++) B.sum[(size_t)k * (size_t)B.cap + (size_t)i] = A.sum[(size_t)k * (size_t)A.cap + (size_t)j];
}

template <typename H>
__device__ __forceinline__ int pa_short(H zlim) {      // min, max, nint of partoutput_average.f90:108-111
  zlim = zlim < (H)32766. ? zlim : (H)32766.;
  zlim = zlim > (H)-32766. ? zlim : (H)-32766.;
  return (int)pa_round(zlim);
}

// partoutput_average.f90:69-198.  out: the file's records, 24 bytes each, zeroed by the caller; a valid particle writes
// the record of its number.  stat[0]: number of valid particles, stat[1]: 1 + the largest valid particle number (0-based).
template <typename R, typename H>
__global__ void __launch_bounds__(256) k_partavg_out(Parts<R> P, State<H> S, long long n, int itime, unsigned int *__restrict__ out,
                                                     unsigned int *__restrict__ stat) {
#pragma clang fp contract(off)
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s < n;                             // no early return: the wave sums its counts below
  const bool valid = live && P.itra1[s] == itime;
  unsigned int last = 0;
  if (valid) {
    const unsigned int pid = P.pid[s];
    last = pid + 1u;
    const H cnt = (H)S.npart_av[s];
    H a[kSums];
#pragma unroll
    for (int k = 0; k < kSums; k++) a[k] = pa_div(S.sum[(size_t)k * (size_t)S.cap + (size_t)s], cnt);
    const H pi180 = pa_div((H)3.14159265, (H)180.);
    H xlon = pa_atan2(a[CARTX], (H)-1. * a[CARTY]);
    H ylat = pa_atan2(a[CARTZ], pa_sqrt(a[CARTX] * a[CARTX] + a[CARTY] * a[CARTY]));
    xlon = pa_div(xlon, pi180);
    ylat = pa_div(ylat, pi180);
    if (xlon > (H)180.) xlon = xlon - (H)360.;
    if (xlon < (H)-180.) xlon = xlon + (H)360.;
    int v[12];
    v[0] = (int)pa_round(xlon * (H)180.);
    v[1] = (int)pa_round(ylat * (H)360.);
    v[2] = pa_short<H>(a[Z] * (H)2. - (H)32000.);
    v[3] = pa_short<H>(a[TOPO] * (H)2. - (H)32000.);
    v[4] = pa_short<H>(a[TRO] * (H)2. - (H)32000.);
    v[5] = pa_short<H>(a[HMIX] * (H)2. - (H)32000.);
    v[6] = pa_short<H>(a[RHO] * (H)20000. - (H)32000.);
    v[7] = pa_short<H>(a[QV] * (H)1000000. - (H)32000.);
    v[8] = pa_short<H>(a[PV] * (H)100.);
    v[9] = pa_short<H>((a[TT] - (H)273.15) * (H)300.);
    v[10] = pa_short<H>(a[UU] * (H)200.);
    v[11] = pa_short<H>(a[VV] * (H)200.);
    unsigned int *w = out + (size_t)pid * 6;
#pragma unroll
    for (int k = 0; k < 6; k++) w[k] = ((unsigned int)v[2 * k] & 0xFFFFu) | ((unsigned int)v[2 * k + 1] << 16);
  }
  if (live) {
    S.npart_av[s] = 0;                                 // :172-186, every space
#pragma unroll
    for (int k = 0; k < kSums; k++) S.sum[(size_t)k * (size_t)S.cap + (size_t)s] = (H)0;
  }
  const unsigned long long m = __ballot(valid);
  for (int o = 32; o > 0; o >>= 1) last = max(last, (unsigned int)__shfl_xor((int)last, o));
  if ((threadIdx.x & 63) == 0 && m) {
    atomicAdd(&stat[0], (unsigned int)__popcll(m));
    atomicMax(&stat[1], last);
  }
}

}  // namespace pa
FPX_TU_CLOSE
}  // namespace fpx
