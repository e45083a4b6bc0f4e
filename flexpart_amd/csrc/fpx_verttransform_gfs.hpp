// Device side of fpx_verttransform_gfs: the reference's verttransform_gfs (src/verttransform_gfs.f90:84-494 -- NCEP GFS
// pressure levels -> terrain-following z levels, rho, drhodz, pplev, w conversion and slope correction, polar-stereographic
// winds) as HIP kernels for gfx950.  The cloud block :498-596 and clwc are not computed.
//
// What differs from verttransform_ecmwf (fpx_verttransform.hpp), by line of the reference:
//   :149-154  the vertical structure of a column starts at its own level llev (the first pressure level above the ground,
//             capped at nuvz-2): uvwzlev(llev) = 0, rhoh(llev) from akz(llev) alone, pinmconv(llev) one-sided, z level 1 is
//             model level llev
//   :214-261  pplev, the pressure on the z levels, interpolated from akz with the weights of u, v, T, q
//   :271-285  w: a z level 2..nz-1 above the column's top is not written -- ww keeps what the slot held before the call
//             (O.ww is the slot's own persistent array) and the slope term :354 is added to that
//   :329-354  the slope term of a z level without bracket uses the bracket of the last z level of the column that had one
//   :453-457  the south pole row: ddpol = pi + atan(u/v) - xlonr for vv > 0
// Design: the host's (ix,jy,level) layout, consecutive lanes on consecutive ix, arithmetic in the host's real kind H with
// FMA contraction off, as in fpx_verttransform.hpp.  GFS has few levels (26-41), so the sequential parts are not cut into
// level-parallel kernels: one lane owns a column and walks its levels, and every access of a wave is a contiguous row
// segment of one level (or of two neighbouring levels where llev differs inside the wave).
//   k_vg_levels (ix,jy)  llev and uvwzlev = the running sum of the layer thicknesses from llev upwards; 0 below llev (the
//                        reference leaves those entries of its automatic array unwritten and the slope term of a
//                        neighbour column may read them)
//   k_vg_column (ix,jy)  one walk over the z levels: the bracket of each level -- one search serves the u/v sweep, the w
//                        sweep (wzlev = uvwzlev here) and the slope sweep, which test the same numbers --, u, v, T, q, pv,
//                        rho, pplev, w, drhodz from the last two rho, the slope term from the neighbour columns' uvwzlev
//   k_vt_polar / k_vg_polerow   the polar caps
// The searches of the reference restart at llev+1 for every z level and do not leave at the first match.  uvwzlev
// increases strictly with the level (every layer thickness is const*log(pold/pint) times a mean virtual temperature, and
// akz decreases), so a z level has one bracket at most and the bracket of the next z level is the same or a higher one:
// the walk resumes at the last bracket and stops at the first match.
#pragma once
#include "fpx_verttransform.hpp"

namespace fpx {
FPX_TU_OPEN
namespace vt {

#define VK(x) ((H)(x))

// :149-154 (= :313-318)
template <typename H>
__device__ __forceinline__ int vg_llev(const H *akz, H p, int nuvz) {
  int llev = 0;
  for (int i = 1; i <= nuvz; i++)
    if (p < akz[i - 1]) llev = i;
  llev = llev + 1;
  if (llev > nuvz - 2) llev = nuvz - 2;
  return llev;
}

// :163-184
template <typename H>
__global__ void __launch_bounds__(256) k_vg_levels(Geo<H> G, In<H> I, Out<H> O) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= G.nx * G.ny) return;
  const int ix = t % G.nx, jy = t / G.nx;
  const int nuvz = G.nuvz;
  const H konst = VK(287.05) / VK(9.81);
  const H p = I.ps[G.at2(ix, jy)];
  const int llev = vg_llev<H>(I.akz, p, nuvz);
  for (int kz = 1; kz <= llev; kz++) O.uvzlev[G.at(ix, jy, kz)] = VK(0.);
  size_t o = G.at(ix, jy, llev);
  H tvold = I.tth[o] * (VK(1.) + VK(0.608) * I.qvh[o]);
  H pold = I.akz[llev - 1];
  H acc = VK(0.);
  for (int kz = llev + 1; kz <= nuvz; kz++) {
    o = G.at(ix, jy, kz);
    const H pint = I.akz[kz - 1] + I.bkz[kz - 1] * p;
    const H tv = I.tth[o] * (VK(1.) + VK(0.608) * I.qvh[o]);
    const H dtv = tv - tvold;
    if ((dtv < 0 ? -dtv : dtv) > VK(0.2)) acc = acc + konst * M<H>::log(pold / pint) * (tv - tvold) / M<H>::log(tv / tvold);
    else acc = acc + konst * M<H>::log(pold / pint) * tv;
    O.uvzlev[o] = acc;
    tvold = tv;
    pold = pint;
  }
}

// :188-359 for one column per lane.  O.ww is the slot's persistent array, pplev the extra GFS output.
template <typename H>
__global__ void __launch_bounds__(256) k_vg_column(Geo<H> G, In<H> I, Out<H> O, H *__restrict__ pplev) {
#pragma clang fp contract(off)
  extern __shared__ unsigned char vt_smem[];
  const int nz = G.nz;                               // = nuvz = nwz
  H *hgt = (H *)vt_smem, *akz = hgt + nz, *bkz = akz + nz, *akn = bkz + nz, *bkn = akn + nz;
  for (int k = threadIdx.x; k < nz; k += blockDim.x) {
    hgt[k] = I.height[k]; akz[k] = I.akz[k]; bkz[k] = I.bkz[k]; akn[k] = I.aknew[k]; bkn[k] = I.bknew[k];
  }
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= G.nx * G.ny) return;
  const int ix = t % G.nx, jy = t / G.nx;
  const size_t col = G.at2(ix, jy), plane = (size_t)G.nxmax * (size_t)G.nymax;
  auto At = [&](int k) -> size_t { return col + plane * (size_t)(k - 1); };
  auto U = [&](int k) -> H { return O.uvzlev[At(k)]; };
  const H r_air = VK(287.05);
  const H p = I.ps[col];
  const int llev = vg_llev<H>(akz, p, nz);
  // pinmconv, :188-198
  auto Pin = [&](int k) -> H {
    if (k == llev) return (U(llev + 1) - U(llev)) / ((akn[llev] + bkn[llev] * p) - (akn[llev - 1] + bkn[llev - 1] * p));
    if (k == nz) return (U(nz) - U(nz - 1)) / ((akn[nz - 1] + bkn[nz - 1] * p) - (akn[nz - 2] + bkn[nz - 2] * p));
    return (U(k + 1) - U(k - 1)) / ((akn[k] + bkn[k] * p) - (akn[k - 2] + bkn[k - 2] * p));
  };
  struct Lev { int k; H t, q, u, v, pv, rh, wp; };   // model level k: T, q, u, v, pv, rhoh and wwh*pinmconv there
  auto load = [&](int k) -> Lev {
    const size_t a = At(k);
    Lev L;
    L.k = k; L.t = I.tth[a]; L.q = I.qvh[a]; L.u = I.uuh[a]; L.v = I.vvh[a]; L.pv = I.pvh[a];
    const H w = I.wwh[a];
    const H pk = k == llev ? akz[k - 1] : akz[k - 1] + bkz[k - 1] * p;      // :164,167 / :170,172
    L.rh = pk / (r_air * (L.t * (VK(1.) + VK(0.608) * L.q)));
    L.wp = w * Pin(k);
    return L;
  };
  const Lev bot = load(llev), top = load(nz);
  const H utop = U(nz);
  {   // z level 1, :204-214, :271
    const size_t o = At(1);
    O.uu[o] = bot.u; O.vv[o] = bot.v; O.tt[o] = bot.t; O.qv[o] = bot.q; O.pv[o] = bot.pv; O.rho[o] = bot.rh;
    pplev[o] = akz[llev - 1];
    O.ww[o] = bot.wp;
  }
  const bool inner = ix >= 1 && ix <= G.nx - 2 && jy >= 1 && jy <= G.ny - 2;
  const H pi180 = VK(3.14159265) / VK(180.);
  const H cosf = M<H>::cos(((H)jy * G.dy + G.ylat0) * pi180);
  Lev cl = bot, cu = bot;
  int kcur = llev + 1;                               // where the walk stands
  H zlo = U(llev), zhi = U(llev + 1);
  bool carry = false;                                // the slope sweep's last bracket of this column, :329-339
  int ckl = 0;
  H cdz1 = VK(0.), cdz2 = VK(0.), cdz = VK(0.);
  H r_m1 = bot.rh, r_m2 = VK(0.);
  for (int iz = 2; iz <= nz; iz++) {
    const size_t o = At(iz);
    const H h = hgt[iz - 1];
    bool found = false;
    {
      H a = zlo, b = zhi;
      for (int k = kcur; ; ) {
        if (h > a && h <= b) { found = true; kcur = k; zlo = a; zhi = b; break; }
        if (k == nz) break;
        k++;
        a = b;
        b = U(k);
      }
    }
    H dz1 = VK(0.), dz2 = VK(0.), dz = VK(1.);
    if (found) {
      dz1 = h - zlo; dz2 = zhi - h; dz = dz1 + dz2;
      if (cu.k == kcur - 1) cl = cu; else if (cl.k != kcur - 1) cl = load(kcur - 1);
      if (cu.k != kcur) cu = load(kcur);
    }
    H uu = VK(0.), vv = VK(0.), rho = VK(0.);
    bool wrote = false;
    if (iz == nz || h > utop) {                      // :215-225, :229-241
      uu = top.u; vv = top.v; rho = top.rh; wrote = true;
      O.uu[o] = uu; O.vv[o] = vv; O.tt[o] = top.t; O.qv[o] = top.q; O.pv[o] = top.pv; O.rho[o] = rho;
      pplev[o] = akz[nz - 1];
    } else if (found) {                              // :243-262
      uu = (cl.u * dz2 + cu.u * dz1) / dz;
      vv = (cl.v * dz2 + cu.v * dz1) / dz;
      rho = (cl.rh * dz2 + cu.rh * dz1) / dz;
      wrote = true;
      O.uu[o] = uu; O.vv[o] = vv;
      O.tt[o] = (cl.t * dz2 + cu.t * dz1) / dz;
      O.qv[o] = (cl.q * dz2 + cu.q * dz1) / dz;
      O.pv[o] = (cl.pv * dz2 + cu.pv * dz1) / dz;
      O.rho[o] = rho;
      pplev[o] = (akz[kcur - 2] * dz2 + akz[kcur - 1] * dz1) / dz;
    }
    if (!wrote) { uu = O.uu[o]; vv = O.vv[o]; rho = O.rho[o]; }   // not reached for finite input (0 < h <= utop has a bracket)
    // w, :271-285: the sweep includes nz and overwrites the explicit value there when it finds a bracket
    H ww;
    if (found) ww = (cl.wp * dz2 + cu.wp * dz1) / dz;
    else if (iz == nz) ww = top.wp;
    else ww = O.ww[o];                               // above the top: what the slot held before this call
    if (inner && iz <= nz - 1) {                     // :324-354
      if (found) { carry = true; ckl = kcur - 1; cdz1 = dz1; cdz2 = dz2; cdz = dz; }
      if (carry) {   // (a column whose z level 2 has no bracket would carry the previous column's: left without the term)
        const H ui = uu * G.dxconst / cosf;
        const H vi = vv * G.dyconst;
        const size_t a = At(ckl), b = At(ckl + 1);
        const H dzdx1 = (O.uvzlev[a + 1] - O.uvzlev[a - 1]) / VK(2.);
        const H dzdx2 = (O.uvzlev[b + 1] - O.uvzlev[b - 1]) / VK(2.);
        const H dzdx = (dzdx1 * cdz2 + dzdx2 * cdz1) / cdz;
        const H dzdy1 = (O.uvzlev[a + G.nxmax] - O.uvzlev[a - G.nxmax]) / VK(2.);
        const H dzdy2 = (O.uvzlev[b + G.nxmax] - O.uvzlev[b - G.nxmax]) / VK(2.);
        const H dzdy = (dzdy1 * cdz2 + dzdy2 * cdz1) / cdz;
        ww = ww + (dzdx * ui + dzdy * vi);
      }
    }
    O.ww[o] = ww;
    {   // drhodz of the level below, :291-297
      const int k = iz - 1;
      const H d = k == 1 ? (rho - r_m1) / (hgt[1] - hgt[0]) : (rho - r_m2) / (hgt[k] - hgt[k - 2]);
      O.drhodz[At(k)] = d;
      if (k == nz - 1) O.drhodz[At(nz)] = d;
    }
    r_m2 = r_m1; r_m1 = rho;
  }
}

// the pole row, :380-426 / :447-493: k_vt_polerow with the GFS formula of the south row (:456, - xlonr for vv > 0)
template <typename H>
__global__ void __launch_bounds__(64) k_vg_polerow(Geo<H> G, Out<H> O, int south) {
#pragma clang fp contract(off)
  extern __shared__ unsigned char vt_smem[];
  H *row = (H *)vt_smem;               // [nx] + 3 results
  const int iz = 1 + blockIdx.x, lane = threadIdx.x;
  const H pi = VK(3.14159265);
  const int jpole = south ? 0 : G.ny - 1, jnext = south ? 1 : G.ny - 2, ic = G.nx / 2 - 1;
  for (int ix = lane; ix < G.nx; ix += 64) row[ix] = O.ww[G.at(ix, jnext, iz)];
  __syncthreads();
  if (lane == 0) {
    H xlon = G.xlon0 + (H)ic * G.dx;
    H xlonr = xlon * pi / VK(180.);
    const H ucen = O.uu[G.at(ic, jpole, iz)], vcen = O.vv[G.at(ic, jpole, iz)];
    const H ffpol = M<H>::sqrt(ucen * ucen + vcen * vcen);
    H ddpol;
    if (vcen < VK(0.)) ddpol = south ? M<H>::atan(ucen / vcen) + xlonr : M<H>::atan(ucen / vcen) - xlonr;
    else if (vcen > VK(0.)) ddpol = pi + M<H>::atan(ucen / vcen) - xlonr;
    else ddpol = pi / VK(2.) - xlonr;
    if (ddpol < VK(0.)) ddpol = VK(2.0) * pi + ddpol;
    if (ddpol > VK(2.0) * pi) ddpol = ddpol - VK(2.0) * pi;
    xlon = VK(180.0);
    xlonr = xlon * pi / VK(180.);
    H uuaux, vvaux, up, vp;
    if (!south) { uuaux = -ffpol * M<H>::sin(xlonr + ddpol); vvaux = -ffpol * M<H>::cos(xlonr + ddpol); }
    else { uuaux = +ffpol * M<H>::sin(xlonr - ddpol); vvaux = -ffpol * M<H>::cos(xlonr - ddpol); }
    cc2gll<H>(G.northpolemap, south ? VK(-90.0) : VK(90.0), xlon, uuaux, vvaux, up, vp);   // :469: northpolemap in the south too
    H wdummy = VK(0.);
    for (int ix = 0; ix < G.nx; ix++) wdummy = wdummy + row[ix];
    wdummy = wdummy / (H)G.nx;
    row[G.nx] = up; row[G.nx + 1] = vp; row[G.nx + 2] = wdummy;
  }
  __syncthreads();
  const H up = row[G.nx], vp = row[G.nx + 1], wd = row[G.nx + 2];
  for (int ix = lane; ix < G.nx; ix += 64) {
    const size_t o = G.at(ix, jpole, iz);
    O.uupol[o] = up;
    O.vvpol[o] = vp;
    O.ww[o] = wd;
  }
}

#undef VK

}  // namespace vt
FPX_TU_CLOSE
}  // namespace fpx
