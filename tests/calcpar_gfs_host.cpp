// TEST INFRASTRUCTURE ONLY.  The column body of flexpart_amd/csrc/fpx_calcpar_gfs.hpp (cpg::calcpar_gfs_column) compiled as
// host code (FPX_CPG_HOST) and run over the columns in the order of the device calls, so that it can be compared with the
// reference bit for bit without a GPU (tests/test_calcpar_gfs.py).  The tropopause of a slot persists between the calls, zero
// at first use, as the engine's per-slot buffer does.
//
// Usage: calcpar_gfs_host <4|8> in.bin out.bin
//   in, out: the files of tests/golden/ref_cpg_driver.f90 (their layout is described there); metdata_format must be 1 (NCEP).
#define FPX_CPG_HOST
#include "../flexpart_amd/csrc/fpx_calcpar_gfs.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace fpx::cpg;

template <typename T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "calcpar_gfs_host: short input\n"); exit(2); }
  return v;
}
template <typename H>
static std::vector<H> narrow(const std::vector<double> &v) { return std::vector<H>(v.begin(), v.end()); }
template <typename H>
static void put(FILE *f, const std::vector<H> &v) {
  std::vector<double> w(v.begin(), v.end());
  fwrite(w.data(), sizeof(double), w.size(), f);
}

template <typename H>
static int run(FILE *f, FILE *fo) {
  const std::vector<int32_t> hi = get<int32_t>(f, 9);
  const int nx = hi[0], ny = hi[1], nz = hi[2], ncalls = hi[6], fmt = hi[7], lsubgrid = hi[8];
  if (fmt != 1) { fprintf(stderr, "calcpar_gfs_host: metdata_format must be 1 (NCEP)\n"); return 2; }
  const std::vector<double> hg = get<double>(f, 4);
  const H dy = (H)hg[1], ylat0 = (H)hg[3];
  const std::vector<H> akz = narrow<H>(get<double>(f, nz)), bkz = narrow<H>(get<double>(f, nz));
  get<double>(f, 2 * (size_t)nz);                       // akm, bkm: the NCEP branch does not read them
  const size_t n2 = (size_t)nx * ny, n3 = n2 * nz;
  const std::vector<H> exc = narrow<H>(get<double>(f, n2));
  std::vector<H> trop[2] = {std::vector<H>(n2, (H)0), std::vector<H>(n2, (H)0)};
  std::vector<H> zlev(n3);
  for (int ic = 0; ic < ncalls; ic++) {
    const int slot = get<int32_t>(f, 1)[0];
    const std::vector<H> ps = narrow<H>(get<double>(f, n2)), tt2 = narrow<H>(get<double>(f, n2)), td2 = narrow<H>(get<double>(f, n2));
    const std::vector<H> str = narrow<H>(get<double>(f, n2)), shf = narrow<H>(get<double>(f, n2)), hmix = narrow<H>(get<double>(f, n2));
    const std::vector<H> tth = narrow<H>(get<double>(f, n3)), qvh = narrow<H>(get<double>(f, n3));
    const std::vector<H> uuh = narrow<H>(get<double>(f, n3)), vvh = narrow<H>(get<double>(f, n3));
    std::vector<H> ust(n2), wst(n2), oli(n2), hm(n2);
    std::vector<H> &tr = trop[slot - 1];
    for (int jy = 0; jy < ny; jy++)
      for (int ix = 0; ix < nx; ix++) {
        const size_t c = (size_t)jy * nx + ix;
        Col<H> C;
        C.uuh = uuh.data(); C.vvh = vvh.data(); C.tth = tth.data(); C.qvh = qvh.data(); C.akz = akz.data(); C.bkz = bkz.data();
        C.zlev = zlev.data(); C.o = c; C.stride = n2; C.nuvz = nz; C.lsubgrid = lsubgrid;
        C.ps = ps[c]; C.tt2 = tt2[c]; C.td2 = td2[c]; C.surfstr = str[c]; C.sshf = shf[c]; C.hmix = hmix[c]; C.excessoro = exc[c];
        C.ylat = ylat0 + (H)jy * dy;
        ColOut<H> O;
        calcpar_gfs_column<H, HostM<H>>(C, O);
        ust[c] = O.ustar; wst[c] = O.wstar; oli[c] = O.oli; hm[c] = O.hmix;
        if (O.have_tropopause) tr[c] = O.tropopause;
      }
    put(fo, ust); put(fo, wst); put(fo, oli); put(fo, hm); put(fo, tr);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: calcpar_gfs_host <4|8> in.bin out.bin\n"); return 2; }
  FILE *f = fopen(argv[2], "rb"), *fo = fopen(argv[3], "wb");
  if (!f || !fo) { fprintf(stderr, "calcpar_gfs_host: cannot open the files\n"); return 2; }
  const int rc = atoi(argv[1]) == 4 ? run<float>(f, fo) : run<double>(f, fo);
  fclose(f);
  fclose(fo);
  return rc;
}
