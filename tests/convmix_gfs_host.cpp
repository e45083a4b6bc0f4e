// TEST INFRASTRUCTURE ONLY.  The sounding body of the GFS convection kernel (cvg::gfs_sounding of
// flexpart_amd/csrc/fpx_convect_gfs.hpp: the function k_conv_column_a_gfs calls per column) compiled for the host, over the
// input file of tests/golden/ref_cvg_driver.f90.
// Usage: convmix_gfs_host 4|8 in.bin out.bin call
//   out: for every column of the grid, in grid order: psconv, pconv(1:nuvz) (pconv(nuvz) = 0: never written), phconv(1:nuvz),
//   dpr, tconv, qconv (1:nuvz-1), all as f8, at the time of call `call` (0-based).
#define FPX_CVG_HOST
#include "../flexpart_amd/csrc/fpx_convect_gfs.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename H>
struct HostIO {
  const H *pp1, *pp2, *tt1, *tt2, *qv1, *qv2;      // this column's level 1 of the six fields
  size_t n2;
  std::vector<double> pconv, phconv, dprv, tconv, qconv;
  void load(int k, int u, H *p1, H *p2, H *t1, H *t2, H *q1, H *q2) const {
    const size_t o = (size_t)(k - 1) * n2;
    p1[u] = pp1[o]; p2[u] = pp2[o]; t1[u] = tt1[o]; t2[u] = tt2[o]; q1[u] = qv1[o]; q2[u] = qv2[o];
  }
  void level(int k, H pc, H tc, H qc) { pconv[k - 1] = pc; tconv[k - 1] = tc; qconv[k - 1] = qc; }
  void half(int k, H ph) { phconv[k - 1] = ph; }
  void dpr(int k, H d) { dprv[k - 1] = d; }
  void top(int k) { pconv[k - 1] = 0.; }             // tconv, qconv(nuvz) are not part of the record
};

static std::vector<double> rd(FILE *f, size_t n) {
  std::vector<double> v(n);
  if (fread(v.data(), 8, n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}

template <typename H>
static int run(FILE *fi, FILE *fo, const int32_t *hdr, int call) {
  const int nx = hdr[0], ny = hdr[1], nz = hdr[2], n = hdr[8], ncalls = hdr[9];
  const size_t n2 = (size_t)nx * ny, n3 = n2 * nz;
  rd(fi, 1);                                             // height(nz)
  std::vector<std::vector<H>> fld;
  for (int i = 0; i < 6; i++) {
    const std::vector<double> v = rd(fi, (i < 3 ? n2 : n3) * 2);
    fld.emplace_back(v.begin(), v.end());                // into the host's real kind, as the driver does
  }
  rd(fi, n2 + 3 * (size_t)n);
  std::vector<int32_t> itimes(ncalls);
  if (fread(itimes.data(), 4, ncalls, fi) != (size_t)ncalls) return 2;
  const int itime = itimes[call];
  const H dt1 = (H)(itime - hdr[6]), dt2 = (H)(hdr[7] - itime);
  const H dtt = (H)1. / (dt1 + dt2);
  for (size_t col = 0; col < n2; col++) {
    HostIO<H> io{fld[5].data() + col, fld[5].data() + n3 + col, fld[3].data() + col, fld[3].data() + n3 + col,
                 fld[4].data() + col, fld[4].data() + n3 + col, n2,
                 std::vector<double>(nz, 0.), std::vector<double>(nz, 0.), std::vector<double>(nz - 1, 0.), std::vector<double>(nz - 1, 0.),
                 std::vector<double>(nz - 1, 0.)};
    const H psconv = (fld[0][col] * dt2 + fld[0][n2 + col] * dt1) * dtt;
    fpx::cvg::gfs_sounding<H>(io, nz, dt1, dt2, dtt, psconv);
    const double ps8 = psconv;
    fwrite(&ps8, 8, 1, fo);
    fwrite(io.pconv.data(), 8, nz, fo);
    fwrite(io.phconv.data(), 8, nz, fo);
    fwrite(io.dprv.data(), 8, nz - 1, fo);
    fwrite(io.tconv.data(), 8, nz - 1, fo);
    fwrite(io.qconv.data(), 8, nz - 1, fo);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  FILE *fi = fopen(argv[2], "rb"), *fo = fopen(argv[3], "wb");
  if (!fi || !fo) return 2;
  int32_t hdr[10];
  if (fread(hdr, 4, 10, fi) != 10) return 2;
  const int rc = argv[1][0] == '4' ? run<float>(fi, fo, hdr, atoi(argv[4])) : run<double>(fi, fo, hdr, atoi(argv[4]));
  fclose(fi);
  fclose(fo);
  return rc;
}
