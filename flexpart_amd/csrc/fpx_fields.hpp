// Field repacking: the host's (x, y, z) arrays of readwind.f90 / verttransform into the device packs (z fastest, the
// variables of one gather interleaved), hmix of a cell's corners (advance.f90:238-252), the wind pack blended in time per
// grid point (interpol_wind.f90:189-191), the level-major copy the convection reads, and conversions between real kinds.
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#include <cstddef>

namespace fpx {
FPX_TU_OPEN

// ---------------------------------------------------------------------------
// field repacking kernels
// ---------------------------------------------------------------------------
// 3-D field (x fastest, strides nxmax,nymax) -> out[((jy*nx+ix)*nz + k)*stride + off]
// (z fastest).  32x32 LDS tile transposes x<->z so both sides move whole rows.
template <typename H, typename R>
__global__ void k_pack3(const H *__restrict__ in, R *__restrict__ out, int nx, int ny, int nz, int nxmax, int nymax,
                        int stride, int off) {
  __shared__ R tile[32][33];
  const int jy = blockIdx.z;
  const int x0 = blockIdx.x * 32, z0 = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int x = x0 + threadIdx.x, z = z0 + r;
    if (x < nx && z < nz) tile[r][threadIdx.x] = (R)in[(size_t)x + (size_t)nxmax * ((size_t)jy + (size_t)nymax * z)];
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    int x = x0 + r, z = z0 + threadIdx.x;
    if (x < nx && z < nz) out[(((size_t)jy * nx + x) * nz + z) * stride + off] = tile[threadIdx.x][r];
  }
}

template <typename H, typename R>
__global__ void k_pack2(const H *__restrict__ in, R *__restrict__ out, int nx, int ny, int nxmax, int stride, int off) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nx * ny) return;
  int ix = i % nx, jy = i / nx;
  out[(size_t)i * stride + off] = (R)in[(size_t)ix + (size_t)nxmax * jy];
}

// hcell[jy][ix] = max of hmix over the cell's corners and both slots: the loop of
// advance.f90:238-252 (start value 0, jyp clamp of :228-231) == initialize.f90:83-90
template <typename R>
__global__ void k_hcell(const R *__restrict__ sfc, R *__restrict__ hcell, int nx, int ny) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nx * ny) return;
  int ix = i % nx, jy = i / nx;
  int ixp = min(ix + 1, nx - 1), jyp = min(jy + 1, ny - 1);
  R h = (R)0;
  for (int s = 0; s < 2; s++) {
    h = fmax(h, sfc[(((size_t)jy * nx + ix) * 2 + s) * 4 + 3]);
    h = fmax(h, sfc[(((size_t)jy * nx + ixp) * 2 + s) * 4 + 3]);
    h = fmax(h, sfc[(((size_t)jyp * nx + ix) * 2 + s) * 4 + 3]);
    h = fmax(h, sfc[(((size_t)jyp * nx + ixp) * 2 + s) * 4 + 3]);
  }
  hcell[i] = h;
}

template <typename S, typename D>
__global__ void k_conv_pack(const S *__restrict__ src, D *__restrict__ dst, int nx, int ny, int nlev, int nxmax, int nymax) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, n2 = (long long)nx * ny;
  if (i >= n2 * nlev) return;
  const int k = (int)(i / n2), r = (int)(i % n2), jy = r / nx, ix = r % nx;
  dst[i] = (D)src[(size_t)ix + (size_t)nxmax * ((size_t)jy + (size_t)nymax * k)];
}

// The wind pack blended in time for the step in flight: out0 at itime, out1 (may be NULL) at itime + lsynctime*ldirect.
// (y(memind(1))*dt2 + y(memind(2))*dt1)*dtt, interpol_wind.f90:189-191, per grid point instead of per particle.
template <typename R>
__global__ void __launch_bounds__(256) k_blend_w3(const R *__restrict__ w3, const R *__restrict__ r2, long long npoint, int m1, int m2, R dt1a, R dt2a, R dtta,
                                                  R dt1b, R dt2b, R dttb, R *__restrict__ out0, R *__restrict__ out1, R *__restrict__ rout0) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npoint) return;
  const R *p = w3 + i * 6;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const R y1 = p[m1 * 3 + k], y2 = p[m2 * 3 + k];
    out0[i * 3 + k] = (y1 * dt2a + y2 * dt1a) * dtta;
    if (out1) out1[i * 3 + k] = (y1 * dt2b + y2 * dt1b) * dttb;
  }
  const R *q = r2 + i * 4;                     // (rho, drhodz) of the two slots, interpol_all.f90:189-198
#pragma unroll
  for (int k = 0; k < 2; k++) rout0[i * 2 + k] = (q[m1 * 2 + k] * dt2a + q[m2 * 2 + k] * dt1a) * dtta;
}

template <typename T>
__global__ void k_convert(const T *__restrict__ src, double *__restrict__ dst64, float *__restrict__ dst32, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (dst64) dst64[i] = (double)src[i];
  if (dst32) dst32[i] = (float)src[i];
}

FPX_TU_CLOSE
}  // namespace fpx
