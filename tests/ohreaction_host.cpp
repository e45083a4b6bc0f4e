// TEST INFRASTRUCTURE ONLY.  The host side of flexpart_amd/csrc/fpx_ohreaction.hpp (oh::Hourly: gethourlyOH with caldate,
// zenithangle, photo_O1D) and its device bodies compiled as host code (FPX_OH_HOST: oh_particle, oh_nearest, the blend of
// k_oh_blend restated over the cells), run in the order of the device calls, so that they can be compared with the reference
// bit for bit without a GPU (tests/test_ohreaction.py).  Dead storage spaces are skipped as the kernel skips them.
//
// Usage: ohreaction_host <4|8> in.bin out.bin [itra1.bin]
//   in, out: the files of tests/golden/ref_oh_driver.f90 (their layout is described there); itra1.bin: i4 itra1(n), which the
//            reference does not look at (all alive without it).  The program prints the branch of every gethourlyOH and
//            "skipped <count>" after every ohreaction.
//        ohreaction_host axis <4|8> v1 v2 ...   prints "ok" or what oh::check_axis finds wrong with the axis.
#define FPX_OH_HOST
#include "../flexpart_amd/csrc/fpx_ohreaction.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

using namespace fpx::oh;

template <typename T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "ohreaction_host: short input\n"); exit(2); }
  return v;
}
template <typename H>
static std::vector<H> narrow(const std::vector<double> &v) { return std::vector<H>(v.begin(), v.end()); }
template <typename H>
static void put(FILE *f, const H *v, size_t n) {
  std::vector<double> w(v, v + n);
  fwrite(w.data(), sizeof(double), n, f);
}

template <typename H>
static int run(FILE *f, FILE *fo, const char *itra1_path) {
  const std::vector<int32_t> hi = get<int32_t>(f, 12);
  const int nx = hi[0], ny = hi[1], nz = hi[2], n = hi[3], nspec = hi[7], ncalls = hi[9], nxn = hi[10], nyn = hi[11];
  const std::vector<double> hg = get<double>(f, 9);
  Hourly<H> S;
  S.nx = hi[4]; S.ny = hi[5]; S.nz = hi[6]; S.ldirect = hi[8]; S.bdate = hg[4];
  const std::vector<H> height = narrow<H>(get<double>(f, nz));
  S.lon = narrow<H>(get<double>(f, S.nx)); S.lat = narrow<H>(get<double>(f, S.ny)); S.alt = narrow<H>(get<double>(f, S.nz));
  S.lonjr = narrow<H>(get<double>(f, 360)); S.latjr = narrow<H>(get<double>(f, 180));
  S.jr = narrow<H>(get<double>(f, (size_t)360 * 180 * 12));
  S.field = narrow<H>(get<double>(f, S.cells() * 12));
  S.prepare();
  const size_t n3 = (size_t)nx * ny * nz;
  std::vector<H> tt[2] = {narrow<H>(get<double>(f, n3)), narrow<H>(get<double>(f, n3))};      // (ix,jy,kz), ix fastest
  std::vector<H> d3(n3 * 6, (H)0);                                                            // the engine's [jy][ix][iz][slot][3]
  for (int m = 0; m < 2; m++)
    for (int k = 0; k < nz; k++)
      for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) d3[((((size_t)j * nx + i) * nz + k) * 2 + m) * 3 + 2] = tt[m][((size_t)k * ny + j) * nx + i];
  const std::vector<double> cc = get<double>(f, nspec), dc = get<double>(f, nspec), nc = get<double>(f, nspec);
  const std::vector<double> xt = get<double>(f, n), yt = get<double>(f, n);
  const std::vector<H> zt = narrow<H>(get<double>(f, n));
  std::vector<H> mass = narrow<H>(get<double>(f, (size_t)n * nspec));                          // [nspec][n]
  std::vector<int32_t> itra1((size_t)n, 0);
  if (itra1_path) {
    FILE *fd = fopen(itra1_path, "rb");
    if (!fd || fread(itra1.data(), 4, n, fd) != (size_t)n) { fprintf(stderr, "ohreaction_host: cannot read itra1\n"); return 2; }
    fclose(fd);
  }
  std::vector<H> top(S.nz), blend(S.cells());
  alt_tops(S.alt.data(), S.nz, top.data());
  Args<H> A;
  memset(&A, 0, sizeof(A));
  A.nxOH = S.nx; A.nyOH = S.ny; A.nzOH = S.nz; A.nztop = S.nz - 1;
  A.oh = blend.data(); A.d3 = d3.data(); A.nx = nx; A.ny = ny; A.nz = nz;
  A.dx = (H)hg[0]; A.dy = (H)hg[1]; A.xlon0 = (H)hg[2]; A.ylat0 = (H)hg[3];
  {   // gridcheck_nests.f90:359-372 in H
    const H dxn = (H)hg[5], dyn = (H)hg[6], xlon0n = (H)hg[7], ylat0n = (H)hg[8];
    A.numbnests = 1;
    A.xres[0] = A.dx / dxn; A.yres[0] = A.dy / dyn;
    const H xaux2 = xlon0n + (H)(nxn - 1) * dxn, yaux2 = ylat0n + (H)(nyn - 1) * dyn;
    A.xl[0] = (xlon0n - A.xlon0) / A.dx; A.xr[0] = (xaux2 - A.xlon0) / A.dx;
    A.yl[0] = (ylat0n - A.ylat0) / A.dy; A.yr[0] = (yaux2 - A.ylat0) / A.dy;
  }
  for (int k = 0; k < nspec; k++)
    if (cc[k] > 0.) { A.spec[A.nreact] = k; A.cc[A.nreact] = (H)cc[k]; A.dc[A.nreact] = (H)dc[k]; A.nc[A.nreact] = (H)nc[k]; A.nreact++; }
  A.small = std::numeric_limits<H>::min();
  for (int ic = 0; ic < ncalls; ic++) {
    const std::vector<int32_t> hc = get<int32_t>(f, 7);
    const int itime = hc[1], ltsample = hc[2];
    if (hc[0] == 0) {
      printf("branch %d\n", S.step(itime));
      put(fo, S.memtime, 2);
      put(fo, S.hourly.data(), S.hourly.size());
      continue;
    }
    const long long interp = (long long)std::llround((H)itime - (H)0.5 * (H)ltsample);
    A.slot = std::llabs((long long)hc[3] - interp) < std::llabs((long long)hc[4] - interp) ? 0 : 1;
    A.tl = (H)std::abs(ltsample);
    const H tnum = (H)itime - S.memtime[0], tden = S.memtime[1] - S.memtime[0];
    for (size_t c = 0; c < S.cells(); c++) {                   // k_oh_blend
      const H a = S.hourly[c], b = S.hourly[S.cells() + c];
      blend[c] = a + (b - a) * tnum / tden;
    }
    int skipped = 0;
    for (int s = 0; s < n; s++) {                              // k_ohreaction
      if (itra1[s] == kOhDead) continue;
      H m[kOhMaxSpec] = {};
      for (int k = 0; k < A.nreact; k++) m[k] = mass[(size_t)A.spec[k] * n + s];
      if (oh_particle<H, H>(A, S.lon.data(), S.lat.data(), top.data(), height.data(), xt[s], yt[s], zt[s], m, nullptr) == 1) { skipped++; continue; }
      for (int k = 0; k < A.nreact; k++) mass[(size_t)A.spec[k] * n + s] = m[k];
    }
    printf("skipped %d\n", skipped);
    put(fo, mass.data(), mass.size());
  }
  return 0;
}

template <typename H>
static int axis(int argc, char **argv) {
  std::vector<H> a;
  for (int i = 3; i < argc; i++) a.push_back((H)atof(argv[i]));
  const char *why = check_axis(a.data(), (int)a.size());
  printf("%s\n", why ? why : "ok");
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "axis") return atoi(argv[2]) == 4 ? axis<float>(argc, argv) : axis<double>(argc, argv);
  if (argc != 4 && argc != 5) { fprintf(stderr, "usage: ohreaction_host <4|8> in.bin out.bin [itra1.bin]\n"); return 2; }
  FILE *f = fopen(argv[2], "rb"), *fo = fopen(argv[3], "wb");
  if (!f || !fo) { fprintf(stderr, "ohreaction_host: cannot open the files\n"); return 2; }
  const int rc = atoi(argv[1]) == 4 ? run<float>(f, fo, argc == 5 ? argv[4] : nullptr) : run<double>(f, fo, argc == 5 ? argv[4] : nullptr);
  fclose(f);
  fclose(fo);
  return rc;
}
