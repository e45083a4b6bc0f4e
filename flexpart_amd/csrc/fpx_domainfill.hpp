// Boundary conditions of a domain-filling run (mdomainfill = 1, 2): boundcond_domainfill.f90:54-573, which
// timemanager.f90:240 calls every time step in place of releaseparticles; run by fpx_boundcond_domainfill.
//
//   k_df_stage1   :63-73    the storage spaces in particle-number order (a grid-stride loop): the two box tests on the particles with
//                           itra1 = itime, the vacancy flag itra1 /= itime (after termination) and the count of the active
//                           particles.  The terminated particle numbers go to a list; nothing is written to the particles.
//   k_df_flux     :95-205, :328-439   one lane per release location: deltaz, boundarea, the level search, uu | vv and rho
//                           in the vertical and in time, fluxofmass, the sign rule, acc_mass (into a second buffer) and mmass
//   k_df_cand     :207-297, :441-531  one lane per candidate (an exclusive scan of mmass in the reference's loop order):
//                           position, PV at the position, the acceptance test, nclass and the mass
//   k_df_cand_seq           the same body, one lane, in candidate order: the parity mode of mdomainfill = 2, where a
//                           candidate's place in the serial ran1 stream depends on the acceptance of all earlier ones
//   k_df_decide             more candidates than vacancies (:307-310)?  The kernels behind it do nothing then.
//   k_df_commit, k_df_place the terminations, and the k-th accepted candidate into the k-th vacant space (:283-303)
// All arithmetic is in the host's real kind H with FMA contraction off, in the reference's grouping; no libm on the
// device (the one cos per boundary row is evaluated by the host in H).  The bodies df_flux and df_candidate compile as host
// code too (FPX_DF_HOST), for checks without a GPU.
#pragma once
#ifndef FPX_DF_HOST
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#define FPX_DF_FN __device__ __forceinline__
#else
#define FPX_DF_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif
#include <cstddef>

namespace fpx {
FPX_TU_OPEN
namespace df {

constexpr int kDead = -999999999;

// one release location of the loops :95-105 / :328-340, in their order
struct Loc {
  int side;   // 0: western / eastern boundary (row = jy), 1: southern / northern (row = ix)
  int row;
  int k;      // 0 | 1: west, east | south, north
  int j;      // 1 .. numcolumn(k, row)
};

// the resident packs (fpx_device.hpp View, fpx_partavg.hpp DiagP) as this routine reads them
template <typename R, typename H>
struct Fields {
  const R *w3;       // [ny][nx][nz][2 slots][3] (uu, vv, ww)
  const R *r2;       // [ny][nx][nz][2 slots][2] (rho, drhodz)
  const H *d3;       // [ny][nx][nz][2 slots][3] (pv, qv, tt)
  const H *height;   // [nz], the host's values (the engine's own copy is in the compute kind)
  int nx, ny, nz;
  int m1, m2;        // physical slot (0 | 1) of memind(1), memind(2)
};

template <typename H>
struct Cfg {
  int nx_we[2], ny_sn[2];
  int nxmax, nymax, maxcolumn;
  int mdomainfill, nclassunc;
  H xmpp;                  // xmassperparticle
  H dx, dy, ylat0;
  H dt1, dt2, dtt;         // :79-81
  H lsync;                 // real(lsynctime)
  H ylat_sn[2], cos_sn[2]; // :334-335 per boundary row, from the host
  const int *nc_we, *nc_sn;   // (2, 0:nymax-1), (2, 0:nxmax-1)
  const H *zc_we, *zc_sn;     // (2, 0:nymax-1, maxcolumn), (2, 0:nxmax-1, maxcolumn)
};

template <typename H>
FPX_DF_FN size_t df_idx(const Cfg<H> &C, const Loc &L, int j) {
  const size_t nrow = (size_t)(L.side == 0 ? C.nymax : C.nxmax);
  return (size_t)L.k + 2 * ((size_t)L.row + nrow * (size_t)(j - 1));
}
template <typename H>
FPX_DF_FN H df_zc(const Cfg<H> &C, const Loc &L, int j) { return (L.side == 0 ? C.zc_we : C.zc_sn)[df_idx(C, L, j)]; }
template <typename H>
FPX_DF_FN int df_nc(const Cfg<H> &C, const Loc &L) { return L.side == 0 ? C.nc_we[L.k + 2 * L.row] : C.nc_sn[L.k + 2 * L.row]; }

// the model level below z (:134-141): the first i in 2..nz with height(i) > z.  fpx_domainfill_init refuses columns that
// reach height(nz), and every ztra1 of a candidate lies below its column's top or below height(nz): always found.
template <typename R, typename H>
FPX_DF_FN int df_level(const Fields<R, H> &F, H z) {
  int indz = F.nz - 1;
  for (int i = 2; i <= F.nz; i++)
    if (F.height[i - 1] > z) { indz = i - 1; break; }
  return indz;
}

// branch counters of a call (tests): see tests/domainfill_ref.py for the names
enum { B_DZ_FIRST = 0, B_DZ_LAST, B_DZ_MID, B_CORNER, B_IN, B_OUT, B_MM2, B_COUNT };

// :107-205 | :342-439 for one location: the new acc_mass, mmass, and acc_mass before the particles are taken off (accmasst)
template <typename R, typename H>
FPX_DF_FN void df_flux(const Fields<R, H> &F, const Cfg<H> &C, const Loc &L, H acc_old, H &acc_new, int &mmass, H &acc_sum, int *branch) {
#ifndef FPX_DF_HOST
#pragma clang fp contract(off)
#endif
  const int j = L.j, nc = df_nc(C, L);
  H deltaz;
  int b;
  if (j == 1) { deltaz = (df_zc(C, L, 2) + df_zc(C, L, 1)) / (H)2.; b = B_DZ_FIRST; }
  else if (j == nc) { deltaz = (df_zc(C, L, j) - df_zc(C, L, j - 2)) / (H)2.; b = B_DZ_LAST; }
  else { deltaz = (df_zc(C, L, j + 1) - df_zc(C, L, j - 1)) / (H)2.; b = B_DZ_MID; }
  if (branch) branch[b]++;
  int ix, jy;
  bool corner;
  H boundarea;
  if (L.side == 0) {
    ix = C.nx_we[L.k]; jy = L.row;
    corner = jy == C.ny_sn[0] || jy == C.ny_sn[1];
    boundarea = corner ? deltaz * (H)111198.5 / (H)2. * C.dy : deltaz * (H)111198.5 * C.dy;
  } else {
    ix = L.row; jy = C.ny_sn[L.k];
    corner = ix == C.nx_we[0] || ix == C.nx_we[1];
    boundarea = corner ? deltaz * (H)111198.5 / (H)2. * C.cos_sn[L.k] * C.dx : deltaz * (H)111198.5 * C.cos_sn[L.k] * C.dx;
  }
  if (branch && corner) branch[B_CORNER]++;
  const H z = df_zc(C, L, j);
  const int indz = df_level(F, z), indzp = indz + 1;
  const H dz1 = z - F.height[indz - 1], dz2 = F.height[indzp - 1] - z;
  const H dz = (H)1. / (dz1 + dz2);
  const int slot[2] = {F.m1, F.m2};
  const int comp = L.side == 0 ? 0 : 1;                   // uu | vv
  H windhl[2], rhohl[2];
  for (int m = 0; m < 2; m++) {
    H windl[2], rhol[2];
    for (int in = 0; in < 2; in++) {
      const size_t cell = ((size_t)jy * F.nx + ix) * F.nz + (size_t)(indz + in - 1);
      windl[in] = (H)F.w3[(cell * 2 + slot[m]) * 3 + comp];
      rhol[in] = (H)F.r2[cell * 4 + slot[m] * 2];
    }
    windhl[m] = (dz2 * windl[0] + dz1 * windl[1]) * dz;
    rhohl[m] = (dz2 * rhol[0] + dz1 * rhol[1]) * dz;
  }
  const H windx = (windhl[0] * C.dt2 + windhl[1] * C.dt1) * C.dtt;
  const H rhox = (rhohl[0] * C.dt2 + rhohl[1] * C.dt1) * C.dtt;
  const H fluxofmass = windx * rhox * boundarea * C.lsync;
  H acc = acc_old;
  bool in;
  if (L.k == 0) { in = fluxofmass >= (H)0.; acc = in ? acc + fluxofmass : (H)0.; }
  else { in = fluxofmass <= (H)0.; acc = in ? acc + (fluxofmass < (H)0. ? -fluxofmass : fluxofmass) : (H)0.; }
  if (branch) branch[in ? B_IN : B_OUT]++;
  acc_sum = acc;
  mmass = 0;
  if (acc >= C.xmpp / (H)2.) {
    mmass = (int)((acc + C.xmpp / (H)2.) / C.xmpp);
    acc = acc - (H)mmass * C.xmpp;
  }
  if (branch && mmass >= 2) branch[B_MM2]++;
  acc_new = acc;
}

// does the candidate draw a uniform for z (:233, :467)?
template <typename H>
FPX_DF_FN bool df_interior(const Cfg<H> &C, const Loc &L) { return L.j != 1 && L.j != df_nc(C, L); }

template <typename H>
struct Cand {
  double x, y;
  H z, pvpart, mass;
  int accepted;   // :281-282
  int zcase;      // 0 first, 1 last, 2 interior
  int corner, south, low, lowpv;
};

// :218-282 | :452-516 for one candidate with its uniforms u0 (the free horizontal coordinate) and u1 (z, interior only)
template <typename R, typename H>
FPX_DF_FN void df_candidate(const Fields<R, H> &F, const Cfg<H> &C, const Loc &L, H u0, H u1, Cand<H> &o) {
#ifndef FPX_DF_HOST
#pragma clang fp contract(off)
#endif
  const int j = L.j, nc = df_nc(C, L);
  H fixed, freec;
  int lo, hi;
  if (L.side == 0) { fixed = (H)C.nx_we[L.k]; lo = C.ny_sn[0]; hi = C.ny_sn[1]; }
  else { fixed = (H)C.ny_sn[L.k]; lo = C.nx_we[0]; hi = C.nx_we[1]; }
  o.corner = 1;
  if (L.row == lo) freec = (H)L.row + (H)0.5 * u0;
  else if (L.row == hi) freec = (H)L.row - (H)0.5 * u0;
  else { freec = (H)L.row + (u0 - (H)0.5); o.corner = 0; }
  const double xt = (double)(L.side == 0 ? fixed : freec), yt = (double)(L.side == 0 ? freec : fixed);
  H zt;
  if (j == 1) { zt = df_zc(C, L, 1) + (df_zc(C, L, 2) - df_zc(C, L, 1)) / (H)4.; o.zcase = 0; }
  else if (j == nc) { zt = ((H)2. * df_zc(C, L, j) + df_zc(C, L, j - 1) + F.height[F.nz - 1]) / (H)4.; o.zcase = 1; }
  else { zt = df_zc(C, L, j - 1) + u1 * (df_zc(C, L, j + 1) - df_zc(C, L, j - 1)); o.zcase = 2; }
  // PV at the position, all four horizontal terms in the reference's order (:239-273)
  const int ixm = (int)xt, jym = (int)yt, ixp = ixm + 1, jyp = jym + 1;
  const H ddx = (H)(xt - (double)(H)ixm), ddy = (H)(yt - (double)(H)jym);
  const H rddx = (H)1. - ddx, rddy = (H)1. - ddy;
  const H p1 = rddx * rddy, p2 = ddx * rddy, p3 = rddx * ddy, p4 = ddx * ddy;
  const int indzm = df_level(F, zt), indzp = indzm + 1;
  const H dz1 = zt - F.height[indzm - 1], dz2 = F.height[indzp - 1] - zt;
  const H dz = (H)1. / (dz1 + dz2);
  const int slot[2] = {F.m1, F.m2};
  auto pv = [&](int i, int jj, int kz, int h) -> H { return F.d3[((((size_t)jj * F.nx + i) * F.nz + (size_t)(kz - 1)) * 2 + h) * 3]; };
  H yh1[2];
  for (int mm = 0; mm < 2; mm++) {
    H y1[2];
    for (int in = 0; in < 2; in++) {
      const int kz = indzm + in, h = slot[mm];
      y1[in] = p1 * pv(ixm, jym, kz, h) + p2 * pv(ixp, jym, kz, h) + p3 * pv(ixm, jyp, kz, h) + p4 * pv(ixp, jyp, kz, h);
    }
    yh1[mm] = (dz2 * y1[0] + dz1 * y1[1]) * dz;
  }
  H pvpart = (yh1[0] * C.dt2 + yh1[1] * C.dt1) * C.dtt;
  // :274 (the particle's latitude, ytra1 is double) | :334 (the boundary row's)
  const H ylat = L.side == 0 ? (H)((double)C.ylat0 + yt * (double)C.dy) : C.ylat_sn[L.k];
  o.south = ylat < (H)0.;
  if (o.south) pvpart = (H)-1. * pvpart;
  o.low = !(zt > (H)3000.);
  o.lowpv = !(pvpart > (H)2.0);                           // pvcrit, par_mod.f90:101
  o.accepted = (!o.low && !o.lowpv) || C.mdomainfill == 1;
  H mass = C.xmpp;
  if (C.mdomainfill == 2) mass = mass * pvpart * (H)48. / (H)29. * (H)60. / (H)1.e9;   // ozonescale = 60, :293-294
  o.x = xt; o.y = yt; o.z = zt; o.pvpart = pvpart; o.mass = mass;
}

// :283-284
template <typename H>
FPX_DF_FN int df_nclass(H u2, int nclassunc) {
  const int n = (int)(u2 * (H)nclassunc) + 1;
  return n < nclassunc ? n : nclassunc;
}

#ifndef FPX_DF_HOST
struct Counters {
  unsigned int nterm;            // terminated by this call
  unsigned int maxpid;           // largest particle number (0-based) a new particle took
  unsigned long long nactive;    // itra1 /= -999999999 among 1..numpart after termination
  // k_df_decide
  int ok;
  unsigned int naccepted, nvacant, consumed;
};

// A grid-stride loop over the spaces; the active particles are counted per lane, summed per wave and per block, and reach
// the counter with one atomic per block: one atomic per wave of a lane-per-space launch is 156 000 adds to one address at
// 1e7 spaces, which took 1.9 ms where the pass itself needs 0.05.
template <typename R>
__global__ void __launch_bounds__(256) k_df_stage1(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, long long numpart, long long scan_n, int itime,
                                                   double x0, double x1, double y0, double y1, int do_x, unsigned int *__restrict__ flags,
                                                   unsigned int *__restrict__ termlist, Counters *__restrict__ cnt) {
  __shared__ unsigned int s_active[4];
  unsigned int mine = 0;
  for (long long pid = (long long)blockIdx.x * blockDim.x + threadIdx.x; pid < scan_n; pid += (long long)gridDim.x * blockDim.x) {
    const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : pid;
    int it = P.itra1[s];
    if (pid < numpart) {
      if (it == itime) {
        const double y = P.yt[s];
        bool out = y > y1 || y < y0;                                   // :65-66
        if (do_x) { const double x = P.xt[s]; out = out || x < x0 || x > x1; }   // :67-69
        if (out) { it = kDead; termlist[atomicAdd(&cnt->nterm, 1u)] = (unsigned int)pid; }
      }
      mine += it != kDead ? 1u : 0u;                                   // :71-72
    }
    flags[pid] = it != itime ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
  if ((threadIdx.x & 63) == 0) s_active[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = s_active[0] + s_active[1] + s_active[2] + s_active[3];
    if (t) atomicAdd(&cnt->nactive, (unsigned long long)t);
  }
}

template <typename R, typename H>
__global__ void __launch_bounds__(256) k_df_flux(Fields<R, H> F, Cfg<H> C, const Loc *__restrict__ locs, int nloc, const H *__restrict__ acc_we_old,
                                                 const H *__restrict__ acc_sn_old, H *__restrict__ acc_we_new, H *__restrict__ acc_sn_new,
                                                 unsigned int *__restrict__ mmass, double *__restrict__ accv) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nloc) return;
  const Loc L = locs[l];
  const size_t a = df_idx(C, L, L.j);
  H acc_new, acc_sum;
  int mm;
  df_flux<R, H>(F, C, L, (L.side == 0 ? acc_we_old : acc_sn_old)[a], acc_new, mm, acc_sum, nullptr);
  (L.side == 0 ? acc_we_new : acc_sn_new)[a] = acc_new;
  mmass[l] = (unsigned int)mm;
  accv[l] = (double)acc_sum;
}

template <typename H>
struct CandOut {
  double *x, *y;
  H *z, *mass;
  int *nclass;
  unsigned int *accepted;   // [ncand + 1], the last one 0: the scan's total
};

FPX_DF_FN int df_loc_of(const unsigned int *__restrict__ first, int nloc, unsigned int c) {
  int lo = 0, hi = nloc;                                  // last l with first[l] <= c
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (first[mid] <= c) lo = mid; else hi = mid; }
  return lo;
}

template <typename H>
FPX_DF_FN void df_store(const CandOut<H> &O, unsigned int c, const Cand<H> &o, int nclass) {
  O.x[c] = o.x; O.y[c] = o.y; O.z[c] = o.z; O.mass[c] = o.mass; O.nclass[c] = nclass; O.accepted[c] = o.accepted ? 1u : 0u;
}

// uni: [3][ncand] from the serial stream (parity mode, mdomainfill = 1), or NULL: three uniforms of the candidate's own,
// Philox keyed on (seed; location, m, itime, a tag for this routine)
template <typename R, typename H>
__global__ void __launch_bounds__(256) k_df_cand(Fields<R, H> F, Cfg<H> C, const Loc *__restrict__ locs, const unsigned int *__restrict__ first, int nloc,
                                                 unsigned int ncand, const H *__restrict__ uni, int itime, unsigned long long seed, CandOut<H> O) {
  const unsigned int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncand) return;
  const int l = df_loc_of(first, nloc, c);
  const Loc L = locs[l];
  H u[3];
  if (uni) {
#pragma unroll
    for (int d = 0; d < 3; d++) u[d] = uni[(size_t)d * ncand + c];
  } else {
    unsigned int o[4];
    philox4x32((unsigned int)l, 0x4446494cu /* "DFIL" */, c - first[l], (unsigned int)itime, (unsigned int)seed, (unsigned int)(seed >> 32), o);
#pragma unroll
    for (int d = 0; d < 3; d++) u[d] = (H)((float)(o[d] >> 8) * (1.0f / 16777216.0f));
  }
  Cand<H> o;
  df_candidate<R, H>(F, C, L, u[0], u[1], o);
  df_store<H>(O, c, o, df_nclass<H>(u[2], C.nclassunc));
}

// parity mode of mdomainfill = 2: `stream` holds the next 3 ncand uniforms of the serial stream; a candidate takes one,
// one more at an interior height, one more if it is accepted
template <typename R, typename H>
__global__ void k_df_cand_seq(Fields<R, H> F, Cfg<H> C, const Loc *__restrict__ locs, const unsigned int *__restrict__ first, int nloc, unsigned int ncand,
                              const H *__restrict__ stream, CandOut<H> O, Counters *__restrict__ cnt) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  unsigned int off = 0;
  int l = 0;
  for (unsigned int c = 0; c < ncand; c++) {
    while (l + 1 < nloc && first[l + 1] <= c) l++;
    const Loc L = locs[l];
    const bool interior = df_interior(C, L);
    const H u0 = stream[off], u1 = interior ? stream[off + 1] : (H)0;
    off += interior ? 2u : 1u;
    Cand<H> o;
    df_candidate<R, H>(F, C, L, u0, u1, o);
    int nclass = 0;
    if (o.accepted) nclass = df_nclass<H>(stream[off++], C.nclassunc);
    df_store<H>(O, c, o, nclass);
  }
  cnt->consumed = off;
}

// :307-310: a candidate -- accepted or not -- that finds no vacant storage space stops the reference.  The number of
// accepted candidates before a candidate grows with the candidate, so the last one decides.
__global__ void k_df_decide(const unsigned int *__restrict__ flags, const unsigned int *__restrict__ rank, long long scan_n,
                            const unsigned int *__restrict__ arank, unsigned int ncand, Counters *__restrict__ cnt) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned int nvac = scan_n > 0 ? rank[scan_n - 1] + flags[scan_n - 1] : 0u;
  cnt->nvacant = nvac;
  cnt->naccepted = ncand ? arank[ncand] : 0u;
  cnt->ok = ncand == 0 || arank[ncand - 1] < nvac;
}

template <typename R>
__global__ void __launch_bounds__(256) k_df_commit(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, const unsigned int *__restrict__ termlist,
                                                   const Counters *__restrict__ cnt) {
  if (!cnt->ok) return;
  const unsigned int n = cnt->nterm;
  for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned int pid = termlist[i];
    P.itra1[slot_of_pid ? (long long)slot_of_pid[pid] : (long long)pid] = kDead;
  }
}

// :283-303 for the accepted candidates; species above 1 stay as the storage space's last owner left them
template <typename R, typename H>
__global__ void __launch_bounds__(256) k_df_place(Parts<R> P, const unsigned int *__restrict__ slot_of_pid, CandOut<H> O, const unsigned int *__restrict__ arank,
                                                  const unsigned int *__restrict__ target, unsigned int ncand, int itime, int numparticlecount0, int mintime,
                                                  int ldirect, int itsplit, Counters *__restrict__ cnt) {
  const unsigned int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncand || !cnt->ok || !O.accepted[c]) return;
  const unsigned int k = arank[c], pid = target[k];
  const long long s = slot_of_pid ? (long long)slot_of_pid[pid] : (long long)pid;
  P.xt[s] = O.x[c]; P.yt[s] = O.y[c]; P.zt[s] = (R)O.z[c];
  P.nclass[s] = O.nclass[c];
  P.npoint[s] = numparticlecount0 + (int)k + 1;
  P.idt[s] = mintime; P.itra1[s] = itime; P.itramem[s] = itime;
  P.itrasplit[s] = itime + ldirect * itsplit;
  P.xmass1[s] = (R)O.mass[c];
  atomicMax(&cnt->maxpid, pid);
}
#endif  // FPX_DF_HOST

}  // namespace df
FPX_TU_CLOSE
}  // namespace fpx
