// Storage order of the particles: particle number <-> device slot (upload, download, fill), the locality sort of the
// slots by grid cell and level with its permutation kernels, and the counters of the step's work list after the sort by
// stability class.  The reference keeps particles in release order (releaseparticles.f90); the order here is the
// device's own and never shows in a result.
#pragma once
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include <hip/hip_runtime.h>
#include "fpx_step_common.hpp"
#include <cstddef>

namespace fpx {
FPX_TU_OPEN

// ---------------------------------------------------------------------------
// particle I/O kernels: host order (pid) <-> device slots
// ---------------------------------------------------------------------------
template <typename S, typename D>
__global__ void k_scatter_in(const S *__restrict__ src, D *__restrict__ dst, const unsigned int *__restrict__ slot_of_pid,
                             long long first, long long count) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  long long slot = slot_of_pid ? (long long)slot_of_pid[first + i] : first + i;
  dst[slot] = (D)src[i];
}
template <typename S, typename D>
__global__ void k_gather_out(const S *__restrict__ src, D *__restrict__ dst, const unsigned int *__restrict__ slot_of_pid,
                             long long first, long long count) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  long long slot = slot_of_pid ? (long long)slot_of_pid[first + i] : first + i;
  dst[i] = (D)src[slot];
}
template <typename D>
__global__ void k_fill(D *__restrict__ dst, D val, long long first, long long count, const unsigned int *__restrict__ slot_of_pid) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  long long slot = slot_of_pid ? (long long)slot_of_pid[first + i] : first + i;
  dst[slot] = val;
}
__global__ void k_iota_pid(unsigned int *__restrict__ pid, long long first, long long count) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  pid[first + i] = (unsigned int)(first + i);
}

// ---------------------------------------------------------------------------
// locality sort: key = (jy, ix, level), the order in which the packed fields lie in
// HBM; dead particles sort to the end.  Keeps waves homogeneous (same cell => same
// mixing height, stability regime and similar sub-step counts) and turns the field
// gathers of a wave into a few shared cache lines.
// ---------------------------------------------------------------------------
template <typename R>
__global__ void k_sort_keys(View<R> V, Parts<R> P, long long n, unsigned int *__restrict__ keys, unsigned int *__restrict__ vals,
                            unsigned int dead_key) {
  __shared__ R hgt[kMaxNz];
  for (int k = threadIdx.x; k < V.nz; k += blockDim.x) hgt[k] = V.height[k];
  __syncthreads();
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned int key = dead_key;
  if (P.itra1[i] != kDead) {
    double xt = P.xt[i], yt = P.yt[i];
    if (xt >= 0. && xt <= (double)V.nxmin1 && yt >= 0. && yt <= (double)V.nymin1) {
      int ix = min((int)xt, V.nx - 1), jy = min((int)yt, V.ny - 1);
      int lev = find_level(hgt, V.nz, P.zt[i]);   // 1 .. nz-1
      key = ((unsigned int)jy * V.nx + ix) * (unsigned int)V.nz + (unsigned int)lev;
    }
  }
  keys[i] = key;
  vals[i] = (unsigned int)i;
}

// keys of the inverse operation: the particle number, so that the sort puts every particle back into the storage space
// of its number (slot = pid)
__global__ void k_sort_keys_pid(const unsigned int *__restrict__ pid, long long n, unsigned int *__restrict__ keys, unsigned int *__restrict__ vals) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = pid[i];
  vals[i] = (unsigned int)i;
}

// out[i] = in[perm[i]] for every particle array at once.  Between two re-sorts a particle stays in or next to its grid
// column, so the sources of neighbouring destination blocks share cache lines: workgroups are dealt to the eight XCDs
// round-robin, therefore block b takes tile (b % 8) * tiles_per_xcd + b / 8 -- each XCD's L2 then sees one contiguous
// eighth of the destination range and every source line is fetched from HBM by one XCD instead of by up to eight.
// The arrays go in four groups, one launch each: the source lines a workgroup touches are shared with its neighbours
// (a grid column's particles are re-shuffled among its levels), and only with a few arrays in flight does that
// working set stay in the 4 MB L2 of an XCD until the neighbours have used it (all 18 arrays in one launch: twice the
// compulsory reads).
template <typename R, int GROUP>
__global__ void k_permute(Parts<R> A, Parts<R> B, const unsigned int *__restrict__ perm, long long n, int nspec, int tiles_per_xcd) {
  const long long tile = (long long)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
  long long i = tile * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned int j = perm[i];
  if (GROUP == 0) { B.xt[i] = A.xt[j]; B.yt[i] = A.yt[j]; B.zt[i] = A.zt[j]; B.idt[i] = A.idt[j]; }
  if (GROUP == 1) { B.up[i] = A.up[j]; B.vp[i] = A.vp[j]; B.wp[i] = A.wp[j]; B.itra1[i] = A.itra1[j]; }
  if (GROUP == 2) { B.us[i] = A.us[j]; B.vs[i] = A.vs[j]; B.ws[i] = A.ws[j]; B.itramem[i] = A.itramem[j]; }
  if (GROUP == 3) {
    B.npoint[i] = A.npoint[j]; B.nclass[i] = A.nclass[j]; B.cbt[i] = A.cbt[j]; B.itrasplit[i] = A.itrasplit[j];
    B.pid[i] = A.pid[j];
    for (int ks = 0; ks < nspec; ks++) B.xmass1[(size_t)ks * B.cap + i] = A.xmass1[(size_t)ks * A.cap + j];
    if (A.xscav) for (int ks = 0; ks < nspec; ks++) B.xscav[(size_t)ks * B.cap + i] = A.xscav[(size_t)ks * A.cap + j];
  }
}

// A permutation without locality (the first sort of a freshly seeded or uploaded cloud) would fetch one memory
// transaction per 8-byte element through the direct gather (18 arrays: > 1 kB per particle).  Such a permutation goes
// through one 128-byte record per particle instead: pack (coalesced reads, whole-line writes), then gather whole
// lines and store coalesced.  Species beyond the first keep the direct gather.
template <typename R>
struct alignas(128) SortRecord {
  double xt, yt;
  R v[8];                // zt up vp wp us vs ws xmass1(1)
  int i[6];              // idt itra1 itramem npoint nclass itrasplit
  unsigned int pid;
  int cbt;
};
template <typename R>
__global__ void k_permute_pack(Parts<R> A, SortRecord<R> *__restrict__ rec, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  SortRecord<R> r;
  r.xt = A.xt[i]; r.yt = A.yt[i];
  r.v[0] = A.zt[i]; r.v[1] = A.up[i]; r.v[2] = A.vp[i]; r.v[3] = A.wp[i]; r.v[4] = A.us[i]; r.v[5] = A.vs[i]; r.v[6] = A.ws[i];
  r.v[7] = A.xmass1[i];
  r.i[0] = A.idt[i]; r.i[1] = A.itra1[i]; r.i[2] = A.itramem[i]; r.i[3] = A.npoint[i]; r.i[4] = A.nclass[i]; r.i[5] = A.itrasplit[i];
  r.pid = A.pid[i]; r.cbt = A.cbt[i];
  rec[i] = r;
}
template <typename R>
__global__ void k_permute_unpack(const SortRecord<R> *__restrict__ rec, Parts<R> A, Parts<R> B, const unsigned int *__restrict__ perm,
                                 long long n, int nspec) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned int j = perm[i];
  const SortRecord<R> r = rec[j];
  B.xt[i] = r.xt; B.yt[i] = r.yt;
  B.zt[i] = r.v[0]; B.up[i] = r.v[1]; B.vp[i] = r.v[2]; B.wp[i] = r.v[3]; B.us[i] = r.v[4]; B.vs[i] = r.v[5]; B.ws[i] = r.v[6];
  B.xmass1[i] = r.v[7];
  B.idt[i] = r.i[0]; B.itra1[i] = r.i[1]; B.itramem[i] = r.i[2]; B.npoint[i] = r.i[3]; B.nclass[i] = r.i[4]; B.itrasplit[i] = r.i[5];
  B.pid[i] = r.pid; B.cbt[i] = (short)r.cbt;
  for (int ks = 1; ks < nspec; ks++) B.xmass1[(size_t)ks * B.cap + i] = A.xmass1[(size_t)ks * A.cap + j];
  if (A.xscav) for (int ks = 0; ks < nspec; ks++) B.xscav[(size_t)ks * B.cap + i] = A.xscav[(size_t)ks * A.cap + j];
}
// number of neighbours in the new order whose sources lie more than `window` storage spaces apart
__global__ void k_perm_disorder(const unsigned int *__restrict__ perm, long long n, unsigned int window, unsigned long long *__restrict__ count) {
  __shared__ unsigned int part[kBlock / 64];
  unsigned int mine = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (i > 0) {
      const long long d = (long long)perm[i] - (long long)perm[i - 1];
      mine += (d < 0 ? -d : d) > (long long)window;
    }
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); k++) t += part[k];
    if (t) atomicAdd(count, t);
  }
}

// particle number -> storage space; built on demand (release, splitting, up/download by particle number), not by
// every re-sort: a random 4-byte scatter costs a whole memory transaction per particle
__global__ void k_slot_map(const unsigned int *__restrict__ pid, long long cap, unsigned int *__restrict__ slot_of_pid) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) slot_of_pid[pid[i]] = (unsigned int)i;
}

// After the stable sort of the slots by their 3-bit key: list length = number of keys <= 4 (PBL
// classes), particles due = number of keys <= 6.  One wave, two 64-ary searches (5 dependent
// loads each at 1e8 keys).
__device__ __forceinline__ long long count_le_sorted(const unsigned char *__restrict__ keys, long long lo, long long hi, unsigned char bound) {
  const int lane = threadIdx.x & 63;
  while (hi > lo) {   // keys[< lo] <= bound < keys[>= hi]
    const long long step = (hi - lo + 63) / 64;
    const long long pos = lo + lane * step;
    const bool le = pos < hi && keys[pos] <= bound;
    const int cnt = __popcll(__ballot(le));    // the keys are sorted: the lanes that see <= bound are the first cnt
    if (cnt == 0) { hi = lo; break; }
    const long long nlo = lo + (long long)(cnt - 1) * step + 1;
    const long long nhi = lo + (long long)cnt * step;
    lo = nlo;
    hi = nhi < hi ? nhi : hi;
  }
  return lo;
}
__global__ void k_list_counts(const unsigned char *__restrict__ sorted_keys, long long n, unsigned int *__restrict__ ctr, Stats *st) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  long long upto[5];
  upto[0] = 0;
  for (int c = 1; c <= 4; c++) upto[c] = count_le_sorted(sorted_keys, upto[c - 1], n, (unsigned char)(8 * c - 1));
  const long long npbl = upto[4];
  const long long ndue = count_le_sorted(sorted_keys, npbl, n, kKeyDone);
  if (threadIdx.x == 0) {
    ctr[0] = (unsigned int)npbl;
    for (int c = 1; c <= 4; c++) {
      ctr[kCtrBase + c - 1] = (unsigned int)(upto[c] - upto[c - 1]);
      for (int j = 0; j <= kMaxSlices; j++) ctr[kCtrBase + kCtrStride * j + 8 + c - 1] = (unsigned int)upto[c - 1];
    }
    st->n_due += (unsigned long long)ndue;
  }
}

FPX_TU_CLOSE
}  // namespace fpx
