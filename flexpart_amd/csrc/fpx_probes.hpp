// Diagnostics behind fpx_math_probe, fpx_cbl_probe and fpx_find_level_probe: device functions of fpx_device.hpp (the fp64
// math helpers, hanna.f90 / hanna_short.f90, cbl.f90, the level search of a Langevin pass) on plain arrays, called as the
// step kernels call them, so that tests can pin them one at a time.
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#include "fpx_step_common.hpp"

namespace fpx {
FPX_TU_OPEN

// diagnostics: the fp64 math helpers of fpx_device.hpp on plain arrays (fpx_math_probe)
__global__ void k_math_probe(int fn, const double *__restrict__ x, double *__restrict__ y, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r = 0.0, c, ic2;
  switch (fn) {
    case 0: r = m_expp(v); break;
    case 1: r = m_logp(v); break;
    case 2: r = m_sqrtp(v); break;
    case 3: r = m_rcp(v); break;
    case 4: r = m_rsqrt(v); break;
    case 5: m_cuberoot_parts(v, c, ic2); r = c; break;
    case 7: r = m_erf_e(v, m_expp(-(v * v))); break;
    case 8: r = m_pow08(v); break;
    case 9: r = m_exp_tab(v, &kExpTab[0]); break;
    case 10: r = m_log_abs(v); break;
    case 11: r = m_rcbrt(v); break;
    // 15 .. 18: the raw seeds the root helpers refine -- v_rcp_f64, v_rsq_f64, and the f32 paths of x**(-1/3) and x**(-1/5)
    case 15: r = __builtin_amdgcn_rcp(v); break;
    case 16: r = __builtin_amdgcn_rsq(v); break;
    case 17: r = m_rcbrt_seed(__log2f((float)v)); break;
    case 18: r = m_rfifth_seed(v); break;
    // 19 .. 27, 31: the forms with two quadratic steps, whatever FPX_NEWTON_HW / FPX_NEWTON_F32 make the kernels call
    case 19: r = m_rcp_q2(v); break;
    case 20: r = m_rsqrt_q2(v); break;
    case 21: r = m_sqrtp_q2(v); break;
    case 22: m_sqrt_rsqrt_q2(v, c, ic2); r = c; break;
    case 23: m_sqrt_rsqrt_q2(v, c, ic2); r = ic2; break;
    case 24: r = m_rcbrt_q2(v, m_rcbrt_seed(__log2f((float)v))); break;
    case 25: r = m_pow08_as<false>(v); break;
    case 26: m_cuberoot_parts_as<false>(v, c, ic2); r = c; break;
    case 27: m_cuberoot_parts_as<false>(v, c, ic2); r = ic2; break;
    case 31: r = m_divf_with(3.0, v, m_rcp_q2(v)); break;
    // 28 .. 30: the forms the kernels call that have no number above -- m_sqrt_rsqrt's two results, m_divf as 3/x
    case 28: m_sqrt_rsqrt(v, c, ic2); r = c; break;
    case 29: m_sqrt_rsqrt(v, c, ic2); r = ic2; break;
    case 30: r = m_divf(3.0, v); break;
    case 32: r = m_exp_tab<256, 4>(v, &kExpTab256[0]); break;             // the 256-entry pair of 9 and 14 (the fp64 gas kernels' exponential)
    case 33: r = m_exp_tab_nh<256, 4>(v, &kExpTab256[0]); break;
    // 40 .. 43: the device library's exp and pow as k_ohreaction calls them (fpx_ohreaction.hpp); pow of (x[i], x[n + i])
    case 40: r = exp(v); break;
    case 41: r = (double)expf((float)v); break;
    case 42: r = pow(v, x[n + i]); break;
    case 43: r = (double)powf((float)v, (float)x[n + i]); break;
    default: m_cuberoot_parts(v, c, ic2); r = ic2; break;
  }
  y[i] = r;
}

// diagnostics (fpx_math_probe, fn 12 .. 14): the error function with E = exp(-x*x) handed in, x = in[0 .. n), E = in[n .. 2n) --
// 12: the polynomial form (m_erf_e2), 13: the table form with the table in LDS as in k_pbl_loop (m_erf_tab2); both take the
// point as either member of the pair, which must agree, else NaN -- and 14: exp(-x/2) with the factor in the constants
// (m_exp_tab_nh; x = in[0 .. n) alone).
__global__ void __launch_bounds__(kBlock) k_erf_probe(int fn, const double *__restrict__ in, double *__restrict__ y, long long n) {
  __shared__ __align__(16) double lds_erft[kErfcxIntervals * kErfcxRow];
  for (int k = threadIdx.x; k < kErfcxIntervals * kErfcxRow; k += blockDim.x) lds_erft[k] = kErfcxTab[k];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = in[i];
  if (fn == 14) { y[i] = m_exp_tab_nh(v, &kExpTab[0]); return; }
  const double E = in[n + i];
  const long long j = i + 1 < n ? i + 1 : 0;   // the pair's other member: a neighbour
  const double v2 = in[j], E2 = in[n + j];
  double a, b, c, d;
  if (fn == 12) { m_erf_e2(v, E, v2, E2, a, b); m_erf_e2(v2, E2, v, E, c, d); }
  else { m_erf_tab2(v, E, v2, E2, (lds_erft_ptr)lds_erft, a, b); m_erf_tab2(v2, E2, v, E, (lds_erft_ptr)lds_erft, c, d); }
  const bool same = a == d || (a != a && d != d);
  y[i] = same ? a : __builtin_nan("");
}

// diagnostics (fpx_hanna_probe): hanna() of a Langevin pass on plain arrays, ten values per point -- sigu, sigv, sigw, dsigwdz, 1/tlu,
// 1/tlv, tlw, floored ust, regime, -h/ol > 5.  which = 0: the way the engine goes -- step_invariants() with the plain math as in
// k_prep, packed as the record carries them, through stash slots and StashInv with the stash's LDS tables as in k_pbl_loop;
// which = 1: hanna() as it stands.  One launch per form, so that the compiler cannot share a subexpression between them.
__global__ void __launch_bounds__(kBlock) k_hanna_probe(int which, const double *__restrict__ in, double *__restrict__ out, long long n) {
  __shared__ double slots[(S_ITLU + 1) * kStashStride];
  __shared__ double lds_tab[kLdsTabDoubles];
  for (int k = threadIdx.x; k < kLdsTabDoubles; k += blockDim.x) lds_tab[k] = k < kLdsExpTabAt ? kLogTab[k >> 1][k & 1] : kExpTab[k - kLdsExpTabAt];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double h = in[5 * i], ol = in[5 * i + 1], ust = in[5 * i + 2], wst = in[5 * i + 3], z = in[5 * i + 4];
  double *o = out + 10 * i;
  Turb<double> T;
  T.ol = ol; T.h = h; T.zeta = z / h; T.sigw = 0.; T.dsigwdz = 0.;
  if (which == 0) {
    const Stash<double> S{(Stash<double>::lds_ptr)(slots + threadIdx.x), (lds_tab_ptr)lds_tab};
    const StepInv<double> I = step_invariants(h, ol, ust, wst, PlainMath());
    S.put(S_UST, I.ust); S.put(S_OL, ol); S.put(S_WST2, wst * wst);
    S.put(S_IAUX, I.iaux); S.put(S_SIGU, I.sigu); S.put(S_ITLU, inv_pack_itlu(I));
    const StashInv<double> SI{S};
    T.ust = S.get(S_UST);
    double itlu, itlv;
    hanna(T, z, SI, S, itlu, itlv);
    o[0] = T.sigu; o[1] = T.sigv; o[2] = T.sigw; o[3] = T.dsigwdz; o[4] = itlu; o[5] = itlv; o[6] = T.tlw;
    o[7] = T.ust; o[8] = (double)SI.regime(); o[9] = SI.deep() ? 1. : 0.;
  } else {
    T.ust = ust; T.wst = wst;
    const bool deep = -h / T.ol > 5.;
    hanna(T, z, Stash<double>{nullptr, (lds_tab_ptr)lds_tab});   // (the pass called hanna() with the stash's tables)
    o[0] = T.sigu; o[1] = T.sigv; o[2] = T.sigw; o[3] = T.dsigwdz; o[4] = m_rcp(T.tlu); o[5] = m_rcp(T.tlv); o[6] = T.tlw;
    o[7] = T.ust; o[8] = h / m_abs(ol) < 1. ? 0. : ol < 0. ? 1. : 2.; o[9] = deep ? 1. : 0.;
  }
}

// diagnostics (fpx_cbl_probe): cbl() of a fine sub-step on plain arrays, called as the fp64 gas kernels of k_pbl_loop call it -- a
// StashErfTab over the block's LDS copies of the exp table (the 256-entry one, as there) and the error-function table.  in[10i .. 10i+9] = wp, z (= zp/h), wt
// (= wst^3 * transition), 1/h, rhograd/rhoa, sigmaw, 1/sigmaw, dsigmawdz, tlw, ldirect; out[3i .. 3i+2] = ath, bth, flagrein.
// FORM 0: the body in the reference's dimensional variables, 1: the normalised one; an instance each, whatever FPX_CBL_NORMALISED is.
template <int FORM>
__global__ void __launch_bounds__(kBlock) k_cbl_probe(const double *__restrict__ in, double *__restrict__ out, long long n) {
  __shared__ double lds_tab[lds_tab_doubles(FPX_EXP_TAB_FINE != 0)];
  __shared__ __align__(16) double lds_erft[kErfcxIntervals * kErfcxRow];
  if (FPX_EXP_TAB_FINE) lds_tab_fill_fine(lds_tab);
  else for (int k = threadIdx.x; k < kLdsTabDoubles; k += blockDim.x) lds_tab[k] = k < kLdsExpTabAt ? kLogTab[k >> 1][k & 1] : kExpTab[k - kLdsExpTabAt];
  for (int k = threadIdx.x; k < kErfcxIntervals * kErfcxRow; k += blockDim.x) lds_erft[k] = kErfcxTab[k];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double *x = in + 10 * i;
  const StashErfTab S = make_stash<double, true>(nullptr, (lds_tab_ptr)lds_tab, (lds_erft_ptr)lds_erft);
  double ath = 0., bth = 0.;
  int flagrein = 0;
  cbl<FORM>(S, x[9] < 0. ? -1 : 1, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], ath, bth, flagrein);
  out[3 * i] = ath; out[3 * i + 1] = bth; out[3 * i + 2] = (double)flagrein;
}

// diagnostics (fpx_find_level_probe): the level search of a Langevin pass on plain arrays, the height column in LDS as in k_pbl_loop.
// which = 0: find_level_from with the point's guess (0: none); which = 1: find_level and the two heights the pass read after it.
// One launch per form.  idx[i] = the level, zz[2i], zz[2i+1] = height(indz), height(indz+1).
template <typename R>
__global__ void __launch_bounds__(kBlock) k_find_level_probe(int which, const R *__restrict__ height, int nz, const R *__restrict__ z,
                                                            const int *__restrict__ guess, long long n, int *__restrict__ idx, R *__restrict__ zz) {
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < nz; k += blockDim.x) hgt[k] = height[k];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R zt = z[i];
  R zlo, zhi;
  int k;
  if (which == 0) k = find_level_from(hgt, nz, zt, guess[i], zlo, zhi);
  else { k = find_level(hgt, nz, zt); zlo = hgt[k - 1]; zhi = hgt[k]; }
  idx[i] = k; zz[2 * i] = zlo; zz[2 * i + 1] = zhi;
}

FPX_TU_CLOSE
}  // namespace fpx
