// TEST INFRASTRUCTURE ONLY.  The device bodies of flexpart_amd/csrc/fpx_domainfill.hpp (df_flux, df_candidate, df_nclass)
// compiled as host code (FPX_DF_HOST) and run in the stages of fpx_boundcond_domainfill -- terminate and flag, flux of every
// location, scan of mmass, candidates with their places in the serial ran1 stream, scan of the accepted ones, the k-th accepted
// into the k-th vacant storage space, everything committed only when no candidate is left without a space -- so that the
// bodies and the decomposition can be compared with the reference bit for bit without a GPU (tests/test_domainfill.py).
//
// Usage: domainfill_host in.bin out.bin
//   in:  i4 real bytes (4|8), then the input of tests/golden/ref_bc_driver.f90 (its layout is described there)
//   out: what that driver writes after every call; the program ends with status 1 at the call the reference stops in
//        (nothing of that call is written), and prints the branch counters of df_flux to stdout.
#define FPX_DF_HOST
#include "../flexpart_amd/csrc/fpx_domainfill.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fpx::df;

template <typename T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "domainfill_host: short input\n"); exit(2); }
  return v;
}
template <typename T>
static void put(FILE *f, const std::vector<T> &v) { fwrite(v.data(), sizeof(T), v.size(), f); }
template <typename H>
static std::vector<H> narrow(const std::vector<double> &v) { return std::vector<H>(v.begin(), v.end()); }

// random_mod.f90:12-42 in the kind H
template <typename H>
struct Ran1 {
  int iv[32] = {}, iy = 0, idum = -11;
  H next() {
    const int ia = 16807, im = 2147483647, iq = 127773, ir = 2836, ntab = 32, ndiv = 1 + (im - 1) / ntab;
    const H am = (H)1. / (H)im, rnmx = (H)1. - (H)1.2e-7;
    if (idum <= 0 || iy == 0) {
      idum = std::max(-idum, 1);
      for (int j = ntab + 8; j >= 1; j--) {
        const int k = idum / iq;
        idum = ia * (idum - k * iq) - ir * k;
        if (idum < 0) idum += im;
        if (j <= ntab) iv[j - 1] = idum;
      }
      iy = iv[0];
    }
    const int k = idum / iq;
    idum = ia * (idum - k * iq) - ir * k;
    if (idum < 0) idum += im;
    const int j = 1 + iy / ndiv;
    iy = iv[j - 1];
    iv[j - 1] = idum;
    return std::min(am * (H)iy, rnmx);
  }
};

template <typename H>
static int run(FILE *f, FILE *fo) {
  const std::vector<int32_t> hi = get<int32_t>(f, 24);
  const int nx = hi[0], ny = hi[1], nz = hi[2], cap = hi[3], ncalls = hi[6], lsynctime = hi[8], mdf = hi[13], xglobal = hi[14], gdf = hi[15];
  const int mintime = hi[20], ldirect = hi[21], itsplit = hi[22], mc = hi[23];
  int numpart = hi[4], npc = hi[5], itime = hi[7];
  const int memind[2] = {hi[9], hi[10]}, memtime[2] = {hi[11], hi[12]};
  const std::vector<double> hg = get<double>(f, 4);
  const std::vector<H> height = narrow<H>(get<double>(f, nz));
  const size_t n3 = (size_t)nx * ny * nz;
  std::vector<H> w3(n3 * 6, (H)0), r2(n3 * 4, (H)0), d3(n3 * 6, (H)0);
  for (int m = 0; m < 2; m++)
    for (int fld = 0; fld < 4; fld++) {                    // uu, vv, rho, pv as (ix,jy,kz) into the packs' [jy][ix][kz][slot][..]
      const std::vector<double> a = get<double>(f, n3);
      for (int kz = 0; kz < nz; kz++)
        for (int jy = 0; jy < ny; jy++)
          for (int ix = 0; ix < nx; ix++) {
            const H v = (H)a[((size_t)kz * ny + jy) * nx + ix];
            const size_t cell = ((size_t)jy * nx + ix) * nz + kz;
            if (fld < 2) w3[(cell * 2 + m) * 3 + fld] = v;
            else if (fld == 2) r2[cell * 4 + m * 2] = v;
            else d3[(cell * 2 + m) * 3] = v;
          }
    }
  const std::vector<int32_t> nc_we = get<int32_t>(f, 2 * ny), nc_sn = get<int32_t>(f, 2 * nx);
  const std::vector<H> zc_we = narrow<H>(get<double>(f, (size_t)2 * ny * mc)), zc_sn = narrow<H>(get<double>(f, (size_t)2 * nx * mc));
  std::vector<H> acc_we = narrow<H>(get<double>(f, (size_t)2 * ny * mc)), acc_sn = narrow<H>(get<double>(f, (size_t)2 * nx * mc));
  std::vector<double> xt = get<double>(f, cap), yt = get<double>(f, cap);
  std::vector<H> zt = narrow<H>(get<double>(f, cap)), xm = narrow<H>(get<double>(f, cap));
  std::vector<int32_t> itra1 = get<int32_t>(f, cap), itramem = get<int32_t>(f, cap), npoint = get<int32_t>(f, cap), nclass = get<int32_t>(f, cap),
                       idt = get<int32_t>(f, cap), itrasplit = get<int32_t>(f, cap);
  Fields<H, H> F{w3.data(), r2.data(), d3.data(), height.data(), nx, ny, nz, memind[0] - 1, memind[1] - 1};
  Cfg<H> C;
  C.nx_we[0] = hi[16]; C.nx_we[1] = hi[17]; C.ny_sn[0] = hi[18]; C.ny_sn[1] = hi[19];
  C.nxmax = nx; C.nymax = ny; C.maxcolumn = mc; C.mdomainfill = mdf; C.nclassunc = 1;
  C.dx = (H)hg[0]; C.dy = (H)hg[1]; C.ylat0 = (H)hg[2]; C.xmpp = (H)hg[3];
  C.lsync = (H)lsynctime;
  for (int k = 0; k < 2; k++) {
    C.ylat_sn[k] = C.ylat0 + (H)C.ny_sn[k] * C.dy;
    C.cos_sn[k] = (H)std::cos(C.ylat_sn[k] * ((H)3.14159265 / (H)180.));
  }
  C.nc_we = nc_we.data(); C.nc_sn = nc_sn.data(); C.zc_we = zc_we.data(); C.zc_sn = zc_sn.data();
  std::vector<Loc> locs;
  for (int side = 0; side < 2; side++) {
    const int lo = side == 0 ? C.ny_sn[0] : C.nx_we[0], hi2 = side == 0 ? C.ny_sn[1] : C.nx_we[1];
    for (int row = lo; row <= hi2; row++)
      for (int k = 0; k < 2; k++)
        for (int j = 1; j <= (side == 0 ? nc_we : nc_sn)[k + 2 * row]; j++) locs.push_back(Loc{side, row, k, j});
  }
  Ran1<H> ran;
  int branch[B_COUNT] = {};
  for (int ic = 0; ic < ncalls; ic++) {
    if (!gdf) {
      C.dt1 = (H)(itime - memtime[0]); C.dt2 = (H)(memtime[1] - itime);
      C.dtt = (H)1. / (C.dt1 + C.dt2);
      // stage 1
      std::vector<int> flags(cap), term;
      const bool do_x = !xglobal || C.nx_we[1] != nx - 2;
      for (int p = 0; p < cap; p++) {
        int it = itra1[p];
        if (p < numpart && it == itime) {
          bool out = yt[p] > (double)(H)C.ny_sn[1] || yt[p] < (double)(H)C.ny_sn[0];
          if (do_x) out = out || xt[p] < (double)(H)C.nx_we[0] || xt[p] > (double)(H)C.nx_we[1];
          if (out) { it = kDead; term.push_back(p); }
        }
        flags[p] = it != itime;
      }
      // stage 2
      std::vector<H> new_we = acc_we, new_sn = acc_sn;
      std::vector<int> first(locs.size() + 1, 0);
      for (size_t l = 0; l < locs.size(); l++) {
        const Loc &L = locs[l];
        const size_t a = df_idx(C, L, L.j);
        H an, as;
        int mm;
        df_flux<H, H>(F, C, L, (L.side == 0 ? acc_we : acc_sn)[a], an, mm, as, branch);
        (L.side == 0 ? new_we : new_sn)[a] = an;
        first[l + 1] = first[l] + mm;
      }
      // stage 3 with stage 5: a candidate's uniforms in the serial stream
      const int ncand = first[locs.size()];
      Ran1<H> copy = ran;
      std::vector<Cand<H>> cand(ncand);
      std::vector<int> cls(ncand, 0), arank(ncand + 1, 0);
      for (size_t l = 0; l < locs.size(); l++)
        for (int c = first[l]; c < first[l + 1]; c++) {
          const Loc &L = locs[l];
          const H u0 = copy.next(), u1 = df_interior(C, L) ? copy.next() : (H)0;
          df_candidate<H, H>(F, C, L, u0, u1, cand[c]);
          if (cand[c].accepted) cls[c] = df_nclass<H>(copy.next(), C.nclassunc);
          arank[c + 1] = arank[c] + (cand[c].accepted ? 1 : 0);
        }
      // stage 4
      std::vector<int> target;
      for (int p = 0; p < cap; p++) if (flags[p]) target.push_back(p);
      if (ncand > 0 && arank[ncand - 1] >= (int)target.size()) {   // :307-310
        printf("stopped %d\n", ic);
        return 1;
      }
      for (int p : term) itra1[p] = kDead;
      for (int c = 0; c < ncand; c++) {
        if (!cand[c].accepted) continue;
        const int k = arank[c], p = target[k];
        xt[p] = cand[c].x; yt[p] = cand[c].y; zt[p] = cand[c].z; nclass[p] = cls[c]; npoint[p] = npc + k + 1;
        idt[p] = mintime; itra1[p] = itime; itramem[p] = itime; itrasplit[p] = itime + ldirect * itsplit; xm[p] = cand[c].mass;
        numpart = std::max(numpart, p + 1);
      }
      npc += arank[ncand];
      acc_we = new_we; acc_sn = new_sn; ran = copy;
    }
    const int32_t counts[2] = {numpart, npc};
    fwrite(counts, 4, 2, fo);
    put(fo, itra1); put(fo, itramem); put(fo, npoint); put(fo, nclass); put(fo, idt); put(fo, itrasplit);
    put(fo, xt); put(fo, yt); put(fo, zt); put(fo, xm); put(fo, acc_we); put(fo, acc_sn);
    for (int p = 0; p < cap; p++) if (itra1[p] == itime) itra1[p] = itime + lsynctime;
    itime += lsynctime;
  }
  printf("branches");
  for (int b = 0; b < B_COUNT; b++) printf(" %d", branch[b]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!f || !fo) return 2;
  const std::vector<int32_t> h = get<int32_t>(f, 1);
  const int rc = h[0] == 4 ? run<float>(f, fo) : run<double>(f, fo);
  fclose(fo);
  return rc;
}
