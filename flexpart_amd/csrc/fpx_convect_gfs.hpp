// Device side of the NCEP GFS branch of fpx_convmix: what the reference's convective mixing does differently when
// metdata_format = GRIBFILE_CENTRE_NCEP.  It differs from the ECMWF branch (fpx_convect.hpp) in three places:
//  * the sounding of a column (convmix.f90:180-188): pconv(kz), tconv(kz), qconv(kz), kz = 1 .. nuvz-1, are the time
//    interpolation (a(m1)*dt2 + a(m2)*dt1)*dtt of the z-level fields pplev, tt, qv at level kz -- not the model-level tth, qvh
//    at kz + 1, and no akz + bkz*ps;
//  * the half levels (calcmatrix.f90:72-77): phconv(1) = psconv, phconv(kuvz) = 0.5*(pconv(kuvz) + pconv(kuvz-1)) for
//    kuvz = 2 .. nuvz, dpr(k) = phconv(k) - phconv(k+1);
//  * the nest test without eps (convmix.f90:108-116) -- unreachable: the reference has no GFS nests, fpx_conv_init_gfs is
//    refused once fpx_nests_init has run, and k_conv_mark runs with one domain.
// nconvlev comes from gridcheck_gfs.f90:513-522 (the host's; nuvz - 2 for the standard GFS levels).
// Quirk, reproduced: phconv(nuvz) reads pconv(nuvz), which no GFS run ever writes (convmix.f90:181 stops at nuvz - 1, for
// tconv and qconv too; conv_mod's arrays are static, so the reference reads the zeros its static storage holds).  The engine
// uses 0 for phconv(nuvz) and stores 0 to pconv(nuvz), tconv(nuvz), qconv(nuvz) of the column's scratch vectors (io.top): the
// scratch is not cleared between calls, and redist.f90:74-85 (half_level_heights) reads pconv, tconv, qconv and phconv up to
// kz = nconvtop + 1, which is nuvz when nconvtop = nconvlev + 1 = nuvz - 1 (CONVECT's inb = nconvlev on the standard GFS
// levels).  With the zeros the top half level gets tv = 0.5 * tv1 there, as in the reference.  While nconvtop <= nconvlev no
// result depends on any of it: CONVECT itself reads levels up to nconvlev + 1.
// Everything after the sounding -- qsconv, the hPa copies, CONVECT's first part -- continues as k_conv_column_a does, into the
// same scratch vectors and Cst scalars, so every kernel from k_conv_survivors on runs unchanged.
//
// The sounding body gfs_sounding compiles as host code too (FPX_CVG_HOST; tests/convmix_gfs_host.cpp): it involves no libm.
#pragma once
#ifndef FPX_CVG_HOST
#include "fpx_convect.hpp"
#define FPX_CVG_FN __device__ __forceinline__
#else
#define FPX_CVG_FN inline
#define FPX_TU_OPEN
#define FPX_TU_CLOSE
#endif
#if defined(__clang__)
#define FPX_CVG_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define FPX_CVG_NOCONTRACT
#endif
#include <cstddef>

namespace fpx {
FPX_TU_OPEN
namespace cvg {

constexpr int kBatch = 8;      // levels whose field values are requested together (k_conv_column_a's eight)

// convmix.f90:180-188 + calcmatrix.f90:66-79 (NCEP branch) for one column, level by level, the values carried in registers.
// IO supplies the fields and takes the results:
//   io.load(k, u, p1, p2, t1, t2, q1, q2)   pplev, tt, qv of the slots memind(1), memind(2) at level k (1-based) into entry u
//   io.level(k, pc, tc, qc)                 pconv(k), tconv(k), qconv(k)
//   io.half(k, ph)                          phconv(k)
//   io.dpr(k, d)                            dpr(k)
//   io.top(nuvz)                            pconv, tconv, qconv(nuvz) = 0: what conv_mod's static storage holds (see above)
// phconv(k+1) needs pconv(k+1): a level's half level and dpr are formed one iteration late.
template <typename H, typename IO>
FPX_CVG_FN void gfs_sounding(IO &io, int nuvz, H dt1, H dt2, H dtt, H psconv) {
  FPX_CVG_NOCONTRACT
  io.half(1, psconv);
  H ph_lo = psconv;            // phconv(k-1) while level k is worked on
  H pc_lo = (H)0.;             // pconv(k-1)
  for (int k0 = 1; k0 <= nuvz - 1; k0 += kBatch) {
    H p1[kBatch], p2[kBatch], t1[kBatch], t2[kBatch], q1[kBatch], q2[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int k = k0 + u < nuvz - 1 ? k0 + u : nuvz - 1;
      io.load(k, u, p1, p2, t1, t2, q1, q2);
    }
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int k = k0 + u;
      if (k > nuvz - 1) break;
      const H pc = (p1[u] * dt2 + p2[u] * dt1) * dtt;
      const H tc = (t1[u] * dt2 + t2[u] * dt1) * dtt;
      const H qc = (q1[u] * dt2 + q2[u] * dt1) * dtt;
      io.level(k, pc, tc, qc);
      if (k >= 2) {
        const H ph = (H)0.5 * (pc + pc_lo);          // phconv(k) = 0.5*(pconv(k) + pconv(k-1))
        io.half(k, ph);
        io.dpr(k - 1, ph_lo - ph);
        ph_lo = ph;
      }
      pc_lo = pc;
    }
  }
  const H ph_top = (H)0.5 * ((H)0. + pc_lo);         // phconv(nuvz): pconv(nuvz) is never written -- 0 (see above)
  io.half(nuvz, ph_top);
  io.dpr(nuvz - 1, ph_lo - ph_top);
  io.top(nuvz);
}

#ifndef FPX_CVG_HOST
using namespace conv;
#define CVG_VV(name, i) Sx.vb[((size_t)V_##name * Sx.nv + (size_t)(i)) * kGroup]

template <typename H>
struct DevIO {
  const Scr<H> &Sx;
  const H *pp1, *pp2, *tt1, *tt2, *qv1, *qv2;      // this column's level 1 of the six fields
  size_t n2;
  int nl;
  __device__ __forceinline__ void load(int k, int u, H *p1, H *p2, H *t1, H *t2, H *q1, H *q2) const {
    const size_t o = (size_t)(k - 1) * n2;
    p1[u] = pp1[o]; p2[u] = pp2[o]; t1[u] = tt1[o]; t2[u] = tt2[o]; q1[u] = qv1[o]; q2[u] = qv2[o];
  }
  __device__ __forceinline__ void level(int k, H pc, H tc, H qc) const {
    FPX_CVG_NOCONTRACT
    CVG_VV(pconv, k) = pc;
    CVG_VV(tconv, k) = tc;
    CVG_VV(qconv, k) = qc;
    CVG_VV(qsconv, k) = cp::f_qvsat<H>(pc, tc);
    if (k <= nl + 1) CVG_VV(pconv_hpa, k) = pc / (H)100.;
  }
  __device__ __forceinline__ void half(int k, H ph) const {
    FPX_CVG_NOCONTRACT
    CVG_VV(phconv, k) = ph;
    if (k <= nl + 1) CVG_VV(phconv_hpa, k) = ph / (H)100.;
  }
  __device__ __forceinline__ void dpr(int k, H d) const { CVG_VV(dpr, k) = d; }
  __device__ __forceinline__ void top(int k) const { CVG_VV(pconv, k) = (H)0.; CVG_VV(tconv, k) = (H)0.; CVG_VV(qconv, k) = (H)0.; }
};

// convmix.f90:173-189 (NCEP) + calcmatrix.f90:56-90 (NCEP) + CONVECT up to its early exits, for every column that holds
// particles: k_conv_column_a with the GFS sounding.  F.dom[0].tth / qvh hold the z-level tt / qv of the two slots; pplev of the
// slots memind(1), memind(2) comes as pp1, pp2 (compact [level][jy][ix]).  One domain: the reference has no GFS nests.
template <typename H>
__global__ void __launch_bounds__(64) k_conv_column_a_gfs(Fields<H> F, const H *__restrict__ pp1, const H *__restrict__ pp2, H *__restrict__ vbuf,
                                                          H *__restrict__ cst, int nv, const int *__restrict__ act, int nact,
                                                          unsigned int *__restrict__ alive) {
#pragma clang fp contract(off)
  if ((int)threadIdx.x >= kSerialLanes) return;
  const int c = blockIdx.x * kSerialLanes + threadIdx.x;
  if (c >= nact) return;
  Scr<H> Sx{vbuf, nullptr, nact, c, nv, 0, 0};
  const Dom<H> &D = F.dom[0];
  const int col = act[c];
  const int nl = F.nconvlev;
  const H dt1 = F.dt1, dt2 = F.dt2, dtt = F.dtt;
  const H psconv = (D.ps[F.m1][col] * dt2 + D.ps[F.m2][col] * dt1) * dtt;
  cst[(size_t)C_psconv * nact + c] = psconv;
  cst[(size_t)C_tt2conv * nact + c] = (D.tt2[F.m1][col] * dt2 + D.tt2[F.m2][col] * dt1) * dtt;
  cst[(size_t)C_td2conv * nact + c] = (D.td2[F.m1][col] * dt2 + D.td2[F.m2][col] * dt1) * dtt;
  DevIO<H> io{Sx, pp1 + col, pp2 + col, D.tth[F.m1] + col, D.tth[F.m2] + col, D.qvh[F.m1] + col, D.qvh[F.m2] + col, (size_t)D.nx * D.ny, nl};
  gfs_sounding<H>(io, F.nuvz, dt1, dt2, dtt, psconv);
  CvState<H> st;
  st.nk = 0; st.icb = 0; st.inb = 0; st.iflag = 0; st.plcl = (H)0.;
  st.cbmf = D.cb[col];
  cst[(size_t)C_cbmfold * nact + c] = st.cbmf;
  int dummy = 0;
  const bool go = convect<H, 1>(Sx, nl, F.delt, st, dummy);
  cst[(size_t)C_cbmf * nact + c] = st.cbmf;
  cst[(size_t)C_plcl * nact + c] = st.plcl;
  cst[(size_t)C_nk * nact + c] = (H)st.nk;
  cst[(size_t)C_icb * nact + c] = (H)st.icb;
  cst[(size_t)C_iflag * nact + c] = (H)st.iflag;
  alive[c] = go ? 1u : 0u;
}

// The device-resident path: nlev levels of a host-shaped [nlevmax][nymax][nxmax] array that is already on the device -> compact
// [nlev][ny][nx], same kind.  Tiling of k_pack3 without its transpose: a block owns 32 ix of 8 levels of one row.
template <typename H>
__global__ void __launch_bounds__(256) k_cvg_compact(const H *__restrict__ in, H *__restrict__ out, int nx, int ny, int nlev, int nxmax, int nymax) {
  const int ix = blockIdx.x * 32 + threadIdx.x, k = blockIdx.y * 8 + threadIdx.y, jy = blockIdx.z;
  if (ix >= nx || k >= nlev || jy >= ny) return;
  out[((size_t)k * ny + jy) * nx + ix] = in[((size_t)k * nymax + jy) * nxmax + ix];
}

// fpx_conv_soundings: the sounding the last call of fpx_convmix left in its scratch for the columns col[0 .. nreq); zeros for a
// column the call did not visit.  One block per column; outputs may be null.
template <typename H>
__global__ void k_conv_soundings(const int *__restrict__ col, int ncol, const unsigned int *__restrict__ colflag, const unsigned int *__restrict__ rank,
                                 H *__restrict__ vbuf, const H *__restrict__ cst, int nv, int nact, int nuvz, H *__restrict__ ps_out,
                                 H *__restrict__ pconv_out, H *__restrict__ phconv_out, H *__restrict__ dpr_out, H *__restrict__ tconv_out,
                                 H *__restrict__ qconv_out) {
  const int i = blockIdx.x;
  const int c = col[i];
  const bool on = nact > 0 && c >= 0 && c < ncol && colflag[c];
  const int r = on ? (int)rank[c] : 0;
  const Scr<H> Sx{vbuf, nullptr, nact, r, nv, 0, 0};
  if (threadIdx.x == 0 && ps_out) ps_out[i] = on ? cst[(size_t)C_psconv * nact + r] : (H)0.;
  for (int k = 1 + (int)threadIdx.x; k <= nuvz; k += blockDim.x) {
    if (phconv_out) phconv_out[(size_t)i * nuvz + k - 1] = on ? CVG_VV(phconv, k) : (H)0.;
    if (k > nuvz - 1) continue;
    const size_t o = (size_t)i * (nuvz - 1) + k - 1;
    if (pconv_out) pconv_out[o] = on ? CVG_VV(pconv, k) : (H)0.;
    if (dpr_out) dpr_out[o] = on ? CVG_VV(dpr, k) : (H)0.;
    if (tconv_out) tconv_out[o] = on ? CVG_VV(tconv, k) : (H)0.;
    if (qconv_out) qconv_out[o] = on ? CVG_VV(qconv, k) : (H)0.;
  }
}
#undef CVG_VV
#endif  // FPX_CVG_HOST

}  // namespace cvg
FPX_TU_CLOSE
}  // namespace fpx
