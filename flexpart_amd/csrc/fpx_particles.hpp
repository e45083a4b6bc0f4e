// The life of a particle outside its step: the synthetic cloud of the benchmarks, the TABLE_SEQ classification, release
// and splitting (releaseparticles.f90:133-375, timemanager.f90:473-504), redistribution between ranks (mpi_mod.f90:661-856),
// warm start (readpartpositions.f90:115-148), the binary particle dump (partoutput.f90:63-190) and the live / newest-birth
// counts.
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#include "fpx_step_common.hpp"
#include "fpx_partavg.hpp"
#include <climits>
#include <cstddef>

namespace fpx {
FPX_TU_OPEN

// ---------------------------------------------------------------------------
// synthetic cloud on the device (benchmarks): same SplitMix64 counters and the
// same arithmetic as flexpart_amd/synthetic.py:make_particles
// ---------------------------------------------------------------------------
__device__ __forceinline__ double splitmix_u01(unsigned long long idx1, unsigned long long seed) {
  unsigned long long z = idx1 * 0x9E3779B97F4A7C15ull + seed;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

template <typename R>
__global__ void k_seed(View<R> V, Parts<R> P, long long n, unsigned long long seed, double frac_pbl, double zmax,
                       double lat_margin, int itime0) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  {
#pragma clang fp contract(off)
  const unsigned long long gi = (unsigned long long)i + V.pid_base + 1ull;   // number in the global cloud
  double ux = splitmix_u01(gi, seed + 1), uy = splitmix_u01(gi, seed + 2);
  double uz = splitmix_u01(gi, seed + 3), us = splitmix_u01(gi, seed + 4);
  const double eps = 361.0 / 3.0e5;
  double x = eps + ux * ((double)(V.nx - 1) - 2.0 * eps);
  double y = lat_margin + uy * ((double)(V.ny - 1) - 2.0 * lat_margin);
  int ix = min((int)x, V.nx - 2), jy = min((int)y, V.ny - 2);
  double hloc = (double)V.hcell[(size_t)jy * V.nx + ix];
  double z = us < frac_pbl ? 10.0 + uz * fmax(hloc - 20.0, 1.0) : hloc + 10.0 + uz * (zmax - hloc - 10.0);
  P.xt[i] = x; P.yt[i] = y; P.zt[i] = (R)z;
  P.up[i] = 0; P.vp[i] = 0; P.wp[i] = 0; P.us[i] = 0; P.vs[i] = 0; P.ws[i] = 0;
  P.idt[i] = 0; P.itra1[i] = itime0; P.itramem[i] = itime0; P.npoint[i] = 1; P.nclass[i] = 1; P.itrasplit[i] = V.ldirect * 999999999;   // "never", signed like itra1 + ldirect*itsplit (releaseparticles.f90:181)
  P.cbt[i] = 1; P.pid[i] = (unsigned int)i;
  for (int ks = 0; ks < V.nspec; ks++) P.xmass1[(size_t)ks * P.cap + i] = (R)1;
  if (P.xscav) for (int ks = 0; ks < V.nspec; ks++) P.xscav[(size_t)ks * P.cap + i] = (R)-1;
  }
}

// ---------------------------------------------------------------------------
// TABLE_SEQ helper: which particles are due / new / take initialize()'s CBL draw
// ---------------------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(kBlock) k_classify(View<R> V, Parts<R> P, long long numpart, int itime, unsigned char *__restrict__ flags) {
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  __syncthreads();
  long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= numpart) return;
  unsigned char f = 0;
  if (P.itra1[s] == itime) {
    f |= 1;
    if (P.itramem[s] == itime || itime == 0) {
      f |= 2;
      double xt = P.xt[s], yt = P.yt[s];
      if (xt >= 0. && xt <= (double)V.nxmin1 && yt >= 0. && yt <= (double)V.nymin1)
        if (initialize_needs_cbl_draws(V, hgt, itime, xt, yt, P.zt[s])) f |= 4;
    }
  }
  flags[P.pid[s]] = f;
}

// ---------------------------------------------------------------------------
// partoutput.f90:63-190 -- the binary particle dump.  The device builds the
// record stream of the file (Fortran sequential unformatted: 4-byte length, payload, 4-byte
// length) for the particles due at itime, in particle-number order, in the host's real kind H;
// the host only streams the bytes to disk.  Arithmetic in H with FMA contraction off: the file
// is byte-identical to the reference's.
// ---------------------------------------------------------------------------
// (DiagP and the interpolation itself, po_gather: fpx_partavg.hpp -- shared with the interval averages)

// Both kernels run over the device slots (cell-sorted after a locality sort: coalesced state reads, gathers with
// the locality of the particle step); the file order is the particle number, so the selection flag and the
// record position are indexed by P.pid.
template <typename R>
__global__ void k_po_flags(Parts<R> P, long long n, int itime, unsigned int *__restrict__ flags) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  flags[P.pid[s]] = P.itra1[s] == itime ? 1u : 0u;
}

__device__ __forceinline__ unsigned int *po_put(unsigned int *w, float v) { *w = __float_as_uint(v); return w + 1; }
__device__ __forceinline__ unsigned int *po_put(unsigned int *w, double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  w[0] = (unsigned int)b; w[1] = (unsigned int)(b >> 32);
  return w + 2;
}

template <typename R, typename H>
__global__ void __launch_bounds__(kBlock) k_partoutput(View<R> V, Parts<R> P, DiagP<H> D, const unsigned int *__restrict__ recidx,
                                                       long long n, int itime, unsigned int *__restrict__ out) {
#pragma clang fp contract(off)
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || P.itra1[s] != itime) return;
  const unsigned int pid = P.pid[s];
  const int nspec = V.nspec;
  const int reclen = 8 + (10 + nspec) * (int)sizeof(H);
  const H zt = (H)P.zt[s];
  PoVals<H> o;
  po_gather<R, H, false>(V, D, itime, P.xt[s], P.yt[s], zt, o);
  const H xlon = o.xlon, ylat = o.ylat, topo = o.topo, pvi = o.pvi, qvi = o.qvi, tti = o.tti, rhoi = o.rhoi, hmixi = o.hmixi, tri = o.tri;
  // the record, :177-179 (32-bit words: the payload of an 8-byte build is only 4-byte aligned in the file)
  unsigned int *w = out + (size_t)recidx[pid] * (size_t)(reclen / 4 + 2);
  *w++ = (unsigned int)reclen;
  *w++ = (unsigned int)P.npoint[s];
  w = po_put(w, xlon); w = po_put(w, ylat); w = po_put(w, zt);
  *w++ = (unsigned int)P.itramem[s];
  w = po_put(w, topo); w = po_put(w, pvi); w = po_put(w, qvi); w = po_put(w, rhoi);
  w = po_put(w, hmixi); w = po_put(w, tri); w = po_put(w, tti);
  for (int ks = 0; ks < nspec; ks++) w = po_put(w, (H)P.xmass1[(size_t)ks * P.cap + s]);
  *w++ = (unsigned int)reclen;
}

// ---------------------------------------------------------------------------
// releaseparticles.f90:133-375 and the splitting block timemanager.f90:473-504
// ---------------------------------------------------------------------------
// per release point and call, prepared by the host in the host's real kind H (releaseparticles.f90:63-131)
template <typename H>
struct RelPoints {
  const long long *first;    // [numpoint+1] exclusive prefix of numrel: particle k of this call belongs to point i with first[i] <= k < first[i+1]
  const long long *gfirst;   // [numpoint] number, in the release count of the whole run over ALL ranks, of this rank's first particle of point i
  const H *xp1, *xaux, *yp1, *yaux, *zp1, *zaux;   // [numpoint]
  const H *mass;             // [nspec][numpoint]: xmass(i,k)/real(npart(i))*timecorrect(k)/average_timecorrect
  const short *kindz;        // [numpoint]
  int numpoint;
};

// free[pid] = the storage space of particle number pid+1 is vacant: itra1 /= itime (:135)
template <typename R>
__global__ void k_rel_flags(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, long long cap, int itime, unsigned int *__restrict__ flags) {
  const long long pid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pid >= cap) return;
  const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : pid;
  flags[pid] = P.itra1[s] != itime ? 1u : 0u;
}
// target[k] = particle number (0-based) of the k-th vacant storage space
__global__ void k_rel_targets(const unsigned int *__restrict__ flags, const unsigned int *__restrict__ rank, long long cap, long long ntotal,
                              unsigned int *__restrict__ target) {
  const long long pid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pid >= cap || !flags[pid]) return;
  const unsigned int r = rank[pid];
  if ((long long)r < ntotal) target[r] = (unsigned int)pid;
}

// a nested wind field as releaseparticles reads it (:196-226,231-341): orography and tt of time slot 2 in the host's real
// kind, compact; rho of slot 2 from the nest's gather pack
template <typename R, typename H>
struct RelNests {
  int n;
  H eps;                              // nxmax/3.e5 (:61)
  struct { int nx, ny; H xl, yl, xr, yr, xres, yres; const H *oro, *tt2; const R *r2; } g[kMaxNests];
};

template <typename R, typename H>
__global__ void __launch_bounds__(kBlock) k_release(View<R> V, Parts<R> P, DiagP<H> D, RelNests<R, H> NS, RelPoints<H> RP, const unsigned int *__restrict__ target,
                                                    const unsigned int *__restrict__ slot_of_pid, long long ntotal, int itime,
                                                    const H *__restrict__ uniforms /* [4][ntotal] serial ran1 stream, or NULL: counter RNG */,
                                                    int numparticlecount0, int mintime, int itsplit, int ind_rel, int nclassunc, int mquasilag,
                                                    H *__restrict__ rho_rel, unsigned int *__restrict__ maxpid) {
#pragma clang fp contract(off)
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ntotal) return;
  // release point of particle k: last i with first[i] <= k
  int lo = 0, hi = RP.numpoint;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (RP.first[mid] <= k) lo = mid; else hi = mid; }
  const int i = lo;
  const unsigned int pid = target[k];
  const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : (long long)pid;
  H u[4];
  if (uniforms) {
#pragma unroll
    for (int d = 0; d < 4; d++) u[d] = uniforms[(size_t)d * ntotal + k];
  } else {   // four uniforms in [0,1) keyed on (seed, number of the particle in the run's release count over all ranks)
    unsigned int o[4];
    const unsigned long long gk = (unsigned long long)(RP.gfirst[i] + (k - RP.first[i]));
    philox4x32((unsigned int)gk, 0x52454c45u /* "RELE" */, (unsigned int)(gk >> 32), 0u,
               (unsigned int)V.seed, (unsigned int)(V.seed >> 32), o);
#pragma unroll
    for (int d = 0; d < 4; d++) u[d] = (H)((float)(o[d] >> 8) * (1.0f / 16777216.0f));
  }
  const int nx = V.nx, ny = V.ny, nz = V.nz;
  double xt = (double)(RP.xp1[i] + u[0] * RP.xaux[i]);                       // :139
  if (V.xglobal) {
    if (xt > (double)(H)V.nxmin1) xt = xt - (double)(H)V.nxmin1;
    if (xt < 0.) xt = xt + (double)(H)V.nxmin1;
  }
  const double yt = (double)(RP.yp1[i] + u[1] * RP.yaux[i]);                 // :146
  int nc = (int)(u[2] * (H)nclassunc) + 1;                                   // :168-169
  nc = nc < nclassunc ? nc : nclassunc;
  H zt = RP.zp1[i] + u[3] * RP.zaux[i];                                      // :183
  // the nest we are in (:196-206), grid coordinates and weights (:211-226)
  int ngrid = 0;
  for (int q = NS.n; q >= 1; q--)
    if (xt > (double)(NS.g[q - 1].xl + NS.eps) && xt < (double)(NS.g[q - 1].xr - NS.eps) && yt > (double)(NS.g[q - 1].yl + NS.eps) &&
        yt < (double)(NS.g[q - 1].yr - NS.eps)) { ngrid = q; break; }
  int ix, jy, gnx = nx, gny = ny, gnxmax = D.nxmax, gnymax = D.nymax;
  H ddx, ddy;
  const H *g_oro = D.oro, *g_tt = nullptr;
  const R *g_r2 = V.r2;
  if (ngrid > 0) {
    const auto &N = NS.g[ngrid - 1];
    const H xtn = (H)((xt - (double)N.xl) * (double)N.xres), ytn = (H)((yt - (double)N.yl) * (double)N.yres);
    ix = (int)xtn; jy = (int)ytn;
    ddy = ytn - (H)jy; ddx = xtn - (H)ix;
    gnx = N.nx; gny = N.ny; gnxmax = N.nx + 1; gnymax = N.ny + 1;      // one padding column / row reads as 0
    g_oro = N.oro; g_tt = N.tt2; g_r2 = N.r2;
  } else {
    ix = (int)xt; jy = (int)yt;
    ddy = (H)(yt - (double)(H)jy); ddx = (H)(xt - (double)(H)ix);
  }
  int ixp = ix + 1, jyp = jy + 1;
  // guards (the reference would read outside its arrays): a position on the upper edges
  ix = min(max(ix, 0), gnx - 1); jy = min(max(jy, 0), gny - 1); ixp = min(max(ixp, 0), gnxmax - 1); jyp = min(max(jyp, 0), gnymax - 1);
  const H rddx = (H)1. - ddx, rddy = (H)1. - ddy;
  const H p1 = rddx * rddy, p2 = ddx * rddy, p3 = rddx * ddy, p4 = ddx * ddy;
  // mother: host layout with stride nxmax; nest: compact [nyn][nxn], the padding reads as 0
  auto oro = [&](int a, int b) -> H {
    if (ngrid > 0) return (a >= gnx || b >= gny) ? (H)0 : g_oro[(size_t)a + (size_t)gnx * (size_t)b];
    return g_oro[(size_t)a + (size_t)D.nxmax * (size_t)b];
  };
  const H topo = p1 * oro(ix, jy) + p2 * oro(ixp, jy) + p3 * oro(ix, jyp) + p4 * oro(ixp, jyp);
  // rho(.,.,kz,2): the r2 pack, physical slot 2; tt(.,.,kz,2): component 2 of the d3 pack (mother) / the nest's compact array
  auto rho2 = [&](int a, int b, int kz) -> H { return (a >= gnx || b >= gny) ? (H)0 : (H)g_r2[(((size_t)b * gnx + a) * nz + (kz - 1)) * 4 + 2]; };
  auto tt2 = [&](int a, int b, int kz) -> H {
    if (a >= gnx || b >= gny) return (H)0;
    if (ngrid > 0) return g_tt[(size_t)a + (size_t)gnx * ((size_t)b + (size_t)gny * (size_t)(kz - 1))];
    return D.d3[((((size_t)b * nx + a) * nz + (kz - 1)) * 2 + 1) * 3 + 2];
  };
  const int kz3 = RP.kindz[i];
  if (kz3 == 3) {                                                            // :231-273
    const H presspart = zt;
    H pressold = (H)0;
    for (int kz = 1; kz <= nz; kz++) {
      const H r = p1 * rho2(ix, jy, kz) + p2 * rho2(ixp, jy, kz) + p3 * rho2(ix, jyp, kz) + p4 * rho2(ixp, jyp, kz);
      const H t = p1 * tt2(ix, jy, kz) + p2 * tt2(ixp, jy, kz) + p3 * tt2(ix, jyp, kz) + p4 * tt2(ixp, jyp, kz);
      const H press = r * (H)287.05 * t / (H)100.;
      if (kz == 1) pressold = press;
      if (press < presspart) {
        if (kz == 1) zt = (H)V.height[0] / (H)2.;
        else {
          const H dz1 = pressold - presspart, dz2 = presspart - press;
          zt = ((H)V.height[kz - 2] * dz2 + (H)V.height[kz - 1] * dz1) / (dz1 + dz2);
        }
        break;
      }
      pressold = press;
    }
  }
  if (kz3 == 2) zt = zt - topo;                                              // :278
  if (zt < (H)1.e-6) zt = (H)1.e-6;
  if (zt > (H)V.height[nz - 1] - (H)0.5) zt = (H)V.height[nz - 1] - (H)0.5;
  H rhoout = (H)1.;
  const bool dens = ind_rel == 1 || ind_rel == 3 || ind_rel == 4;
  if (dens) {                                                                // :300-341
    int indz = nz - 1, indzp = nz;
    for (int ii = 2; ii <= nz; ii++)
      if ((H)V.height[ii - 1] > zt) { indz = ii - 1; indzp = ii; break; }
    const H dz1 = zt - (H)V.height[indz - 1], dz2 = (H)V.height[indzp - 1] - zt, dz = (H)1. / (dz1 + dz2);
    H rhoaux[2];
#pragma unroll
    for (int n = 0; n < 2; n++)
      rhoaux[n] = p1 * rho2(ix, jy, indz + n) + p2 * rho2(ixp, jy, indz + n) + p3 * rho2(ix, jyp, indz + n) + p4 * rho2(ixp, jyp, indz + n);
    rhoout = (dz2 * rhoaux[0] + dz1 * rhoaux[1]) * dz;
    if (rho_rel && k == RP.first[i + 1] - 1) rho_rel[i] = rhoout;            // rho_rel(i) keeps the last particle's value
  }
  for (int ks = 0; ks < V.nspec; ks++) {
    H m = RP.mass[(size_t)ks * RP.numpoint + i];
    if (dens) m = m * rhoout;
    P.xmass1[(size_t)ks * P.cap + s] = (R)m;
    if (P.xscav) P.xscav[(size_t)ks * P.cap + s] = (R)-1;      // releaseparticles.f90:167-171: not yet scavenged
  }
  P.xt[s] = xt; P.yt[s] = yt; P.zt[s] = (R)zt;
  P.nclass[s] = nc;
  P.npoint[s] = mquasilag == 0 ? i + 1 : (int)(numparticlecount0 + k + 1);   // :171-175
  P.idt[s] = mintime; P.itra1[s] = itime; P.itramem[s] = itime;
  P.itrasplit[s] = itime + V.ldirect * itsplit;
  // the turbulent state of the storage space is whatever its last owner left; initialize() overwrites it
  // before the first advance() (timemanager.f90:553), as in the reference
  atomicMax(maxpid, pid);
}

// splitting, timemanager.f90:473-504
template <typename R>
__global__ void k_split_flags(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, long long numpart, int itime, int ldirect,
                              unsigned int *__restrict__ flags) {
  const long long pid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pid >= numpart) return;
  const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : pid;
  flags[pid] = (ldirect * itime >= ldirect * P.itrasplit[s]) ? 1u : 0u;
}
template <typename R>
__global__ void k_split(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, const unsigned int *__restrict__ flags,
                        const unsigned int *__restrict__ rank, long long numpart, long long room, int nspec) {
#pragma clang fp contract(off)
  const long long pid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pid >= numpart || !flags[pid] || (long long)rank[pid] >= room) return;
  const long long j = slot_of_pid ? (long long)slot_of_pid[pid] : pid;
  const long long n = numpart + rank[pid];          // storage spaces behind numpart are identity-numbered
  const int itm = P.itramem[j];
  // itrasplit(j) = 2*(itrasplit(j)-itramem(j))+itramem(j), timemanager.f90:486 -- in 64 bits, saturated at the "never" value
  // (the reference's default integer would overflow once the doubled interval passes 2^31 s)
  long long its64 = 2ll * ((long long)P.itrasplit[j] - itm) + itm;
  its64 = its64 > 999999999ll ? 999999999ll : (its64 < -999999999ll ? -999999999ll : its64);
  const int its = (int)its64;
  P.itrasplit[j] = its; P.itrasplit[n] = its;
  P.itramem[n] = itm; P.itra1[n] = P.itra1[j]; P.idt[n] = P.idt[j]; P.npoint[n] = P.npoint[j]; P.nclass[n] = P.nclass[j];
  P.xt[n] = P.xt[j]; P.yt[n] = P.yt[j]; P.zt[n] = P.zt[j];
  P.up[n] = P.up[j]; P.vp[n] = P.vp[j]; P.wp[n] = P.wp[j];
  P.us[n] = P.us[j]; P.vs[n] = P.vs[j]; P.ws[n] = P.ws[j];
  P.cbt[n] = P.cbt[j];
  for (int ks = 0; ks < nspec; ks++) {
    const R m = P.xmass1[(size_t)ks * P.cap + j] / (R)2;
    P.xmass1[(size_t)ks * P.cap + j] = m;
    P.xmass1[(size_t)ks * P.cap + n] = m;
    if (P.xscav) P.xscav[(size_t)ks * P.cap + n] = P.xscav[(size_t)ks * P.cap + j];   // the copy inherits the receptor's scavenged fraction
  }
}

// Particle redistribution between ranks, mpi_mod.f90:661-856 (mpif_redist_part).  The message is what the reference sends,
// in its order, as ONE buffer: nclass, npoint, itra1, idt, itramem, itrasplit (int32[n] each), xtra1, ytra1 (f64[n]), ztra1
// (R[n]), xmass1 (R[nspec][n]).  As in the reference the turbulent velocities, cbt and xscav_frac1 do NOT travel.
template <typename R>
struct RedistBuf {
  int *nclass, *npoint, *itra1, *idt, *itramem, *itrasplit;
  double *xt, *yt;
  R *zt, *xmass;   // xmass: [nspec][n]
  long long n;
  __host__ __device__ static size_t bytes(long long n, int nspec) { return (size_t)n * (6 * 4 + 2 * 8 + (size_t)(1 + nspec) * sizeof(R)); }
  __host__ __device__ static RedistBuf at(void *base, long long n, int nspec) {
    RedistBuf b;
    unsigned char *q = (unsigned char *)base;
    b.xt = (double *)q; q += (size_t)n * 8;            // the 8-byte arrays first: every array stays aligned for any n
    b.yt = (double *)q; q += (size_t)n * 8;
    b.zt = (R *)q; q += (size_t)n * sizeof(R);
    b.xmass = (R *)q; q += (size_t)n * nspec * sizeof(R);
    b.nclass = (int *)q; q += (size_t)n * 4;
    b.npoint = (int *)q; q += (size_t)n * 4;
    b.itra1 = (int *)q; q += (size_t)n * 4;
    b.idt = (int *)q; q += (size_t)n * 4;
    b.itramem = (int *)q; q += (size_t)n * 4;
    b.itrasplit = (int *)q;
    b.n = n;
    return b;
  }
};
// sender, :700-745: the storage spaces ll..ul = numpart-num_trans+1 .. numpart go into the message and are terminated
template <typename R>
__global__ void k_redist_pack(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, long long first_pid, RedistBuf<R> B, int nspec) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n) return;
  const long long pid = first_pid + i;
  const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : pid;
  B.nclass[i] = P.nclass[s]; B.npoint[i] = P.npoint[s]; B.itra1[i] = P.itra1[s]; B.idt[i] = P.idt[s];
  B.itramem[i] = P.itramem[s]; B.itrasplit[i] = P.itrasplit[s];
  B.xt[i] = P.xt[s]; B.yt[i] = P.yt[s]; B.zt[i] = P.zt[s];
  for (int ks = 0; ks < nspec; ks++) B.xmass[(size_t)ks * B.n + i] = P.xmass1[(size_t)ks * P.cap + s];
  P.itra1[s] = kDead;                                  // :744
}
// receiver, :808-835: valid[i] = the i-th received particle is alive at itime ("we may have transferred invalid particles")
__global__ void k_redist_valid(const int *__restrict__ itra1_tmp, long long n, int itime, unsigned int *__restrict__ valid) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) valid[i] = itra1_tmp[i] == itime ? 1u : 0u;
}
// the k-th valid received particle goes into the k-th storage space of 1..maxnumpart with itra1 /= itime (target[k], as
// k_rel_targets builds it); everything else of that space stays what its last owner left
template <typename R>
__global__ void k_redist_unpack(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, RedistBuf<R> B, int nspec, const unsigned int *__restrict__ valid,
                                const unsigned int *__restrict__ vrank, const unsigned int *__restrict__ target, unsigned int *__restrict__ maxpid) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n || !valid[i]) return;
  const unsigned int pid = target[vrank[i]];
  const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : (long long)pid;
  P.itra1[s] = B.itra1[i]; P.npoint[s] = B.npoint[i]; P.nclass[s] = B.nclass[i]; P.idt[s] = B.idt[i];
  P.itramem[s] = B.itramem[i]; P.itrasplit[s] = B.itrasplit[i];
  P.xt[s] = B.xt[i]; P.yt[s] = B.yt[i]; P.zt[s] = B.zt[i];
  for (int ks = 0; ks < nspec; ks++) P.xmass1[(size_t)ks * P.cap + s] = B.xmass[(size_t)ks * B.n + i];
  atomicMax(maxpid, pid);
}

// readpartpositions.f90:115-148 -- warm start: the records of a dump (as partoutput writes them) -> particle SoA.
// One lane per record; arithmetic of the coordinate conversion in the host's real kind H.
template <typename R, typename H>
__global__ void __launch_bounds__(kBlock) k_readpart(Parts<R> P, const unsigned int *__restrict__ raw, long long n, int nspec,
                                                     H dx, H dy, H xlon0, H ylat0, double jul_header, double bdate, int mintime, int itrasplit0,
                                                     const int *__restrict__ nclass_in, int *__restrict__ status /* [0] error, [1] max npoint */) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int reclen = 8 + (10 + nspec) * (int)sizeof(H);
  const unsigned int *w = raw + (size_t)i * (size_t)(reclen / 4 + 2);
  auto get = [&](const unsigned int *q) -> H {
    if (sizeof(H) == 4) return (H)__uint_as_float(q[0]);
    return (H)__longlong_as_double((long long)(((unsigned long long)q[1] << 32) | (unsigned long long)q[0]));
  };
  const int hw = (int)sizeof(H) / 4;
  if ((int)w[0] != reclen || (int)w[reclen / 4 + 1] != reclen) { atomicExch(&status[0], 1); return; }
  const int npoint = (int)w[1];
  const H xlonin = get(w + 2), ylatin = get(w + 2 + hw), zin = get(w + 2 + 2 * hw);
  const int itramem_in = (int)w[2 + 3 * hw];
  if (xlonin == (H)-9999.9) { atomicExch(&status[0], 2); return; }     // a closing record inside the file: several dumps
  P.xt[i] = (double)((xlonin - xlon0) / dx);                              // :121-122
  P.yt[i] = (double)((ylatin - ylat0) / dy);
  P.zt[i] = (R)zin;
  P.npoint[i] = npoint;
  atomicMax(&status[1], npoint);                                          // numparticlecount, :123
  const double julpartin = jul_header + (double)itramem_in / 86400.;      // :140-147
  P.itramem[i] = (int)llround((julpartin - bdate) * (double)(H)86400.);
  P.idt[i] = mintime;
  P.itrasplit[i] = itrasplit0;                                            // :117
  P.itra1[i] = 0;
  P.nclass[i] = nclass_in ? nclass_in[i] : 1;
  P.up[i] = (R)0; P.vp[i] = (R)0; P.wp[i] = (R)0; P.us[i] = (R)0; P.vs[i] = (R)0; P.ws[i] = (R)0;
  P.cbt[i] = 1; P.pid[i] = (unsigned int)i;
  const unsigned int *x = w + 3 + 3 * hw + 7 * hw;
  for (int ks = 0; ks < nspec; ks++) P.xmass1[(size_t)ks * P.cap + i] = (R)get(x + ks * hw);
  if (P.xscav) for (int ks = 0; ks < nspec; ks++) P.xscav[(size_t)ks * P.cap + i] = (R)-1;   // as after a release; the dump does not carry it
}

// live particles (itra1 /= -999999999) among the first n storage spaces: one atomic per block
__global__ void __launch_bounds__(256) k_count_live(const int *__restrict__ itra1, long long n, unsigned long long *__restrict__ out) {
  __shared__ unsigned int part[4];
  unsigned int c = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) c += itra1[i] != kDead;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
}
// the latest time of birth (itramem, in the run's time direction) among the live particles of the first n storage spaces
__global__ void __launch_bounds__(256) k_birth_max(const int *__restrict__ itra1, const int *__restrict__ itramem, long long n, int ldirect, long long *__restrict__ out) {
  long long m = LLONG_MIN;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    if (itra1[i] != kDead) m = max(m, (long long)ldirect * itramem[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m != LLONG_MIN) atomicMax(out, m);
}

FPX_TU_CLOSE
}  // namespace fpx
