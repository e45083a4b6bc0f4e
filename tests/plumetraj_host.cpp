// TEST INFRASTRUCTURE ONLY.  The device body of flexpart_amd/csrc/fpx_plumetraj.hpp compiled as host code (FPX_PT_HOST) and
// run serially, in storage order, with accumulators of the host's real kind H -- the reference's order -- so that the
// per-particle terms, the per-release-point formulas, the decisions and the formatter of the device can be compared with
// the reference byte for byte without a GPU (tests/test_plumetraj.py).  The interpolated topo, pvi, hmixi, tri come from the
// caller (po_gather is device code; tests/test_partoutput.py and tests/test_partavg.py pin it).
//
// Usage: plumetraj_host in.bin > records
//   in: i4 real bytes (4|8), ncluster, npoints; f8 xlon0, ylat0, dx, dy; then per release point i4 j, age, n; f8 xt(n), yt(n);
//       H zt(n), topo(n), pvi(n), hmixi(n), tri(n)
// Each record line is followed by a line "# passes numb(1..ncluster)".
#define FPX_PT_HOST
#include "../flexpart_amd/csrc/fpx_plumetraj.hpp"

#include <cstdint>
#include <cstdlib>
#include <vector>

using namespace fpx::pt;

template <typename T>
static std::vector<T> get(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "plumetraj_host: short input\n"); exit(2); }
  return v;
}

template <typename H>
static int run(FILE *f, int K, int npoints) {
  const std::vector<double> g = get<double>(f, 4);
  const H xlon0 = (H)g[0], ylat0 = (H)g[1], dx = (H)g[2], dy = (H)g[3];
  const H pi180 = pt_pi180<H>();
  for (int p = 0; p < npoints; p++) {
    const std::vector<int32_t> h = get<int32_t>(f, 3);
    const int n = h[2];
    const std::vector<double> xt = get<double>(f, n), yt = get<double>(f, n);
    const std::vector<H> zt = get<H>(f, n), topo = get<H>(f, n), pvi = get<H>(f, n), hmixi = get<H>(f, n), tri = get<H>(f, n);
    Seg<H> S;
    memset(&S, 0, sizeof(S));
    S.n = n; S.clustered = n >= K;
    std::vector<H> xl(n), yl(n), zl(n);
    std::vector<int> ncl(n, 0);
    H s_topo = 0, s_hmix = 0, s_pv = 0, s_tropo = 0;
    int c_hmix = 0, c_pv = 0, c_tropo = 0;
    for (int i = 0; i < n; i++) {
      xl[i] = pt_lonlat<H>(xlon0, dx, xt[i]);
      yl[i] = pt_lonlat<H>(ylat0, dy, yt[i]);
      const int fl = pt_flags<H>(yl[i], zt[i], pvi[i], tri[i], hmixi[i]);
      c_hmix += fl & 1; c_pv += (fl >> 1) & 1; c_tropo += (fl >> 2) & 1;
      s_topo = s_topo + topo[i]; s_hmix = s_hmix + hmixi[i]; s_pv = s_pv + pvi[i];
      s_tropo = s_tropo + tri[i] + topo[i];
      zl[i] = zt[i] + topo[i];
    }
    if (S.clustered) {
      for (int j = 0; j < K; j++) {
        const int e = (j + 1) * n / K - 1;
        S.xc[j] = xl[e] * pi180; S.yc[j] = yl[e] * pi180;
      }
      S.rmsold = (H)-5.;
      for (int l = 1; l <= kMaxSweeps; l++) {
        Cent<H> cent[kMaxCluster];
        for (int j = 0; j < K; j++) pt_cent<H>(cent[j], S.xc[j], S.yc[j]);
        H a[kMaxQ];
        for (int q = 0; q < kMaxQ; q++) a[q] = (H)0;
        int cnt[kMaxCluster] = {};
        for (int i = 0; i < n; i++) {
          H d, x, y, z;
          const int m = pt_assign<H>(K, cent, xl[i] * pi180, yl[i] * pi180, d, x, y, z);
          ncl[i] = m;
          cnt[m]++;
          a[kSweepQ * K] = a[kSweepQ * K] + d * d;
          a[kSweepQ * m + 1] = a[kSweepQ * m + 1] + d * d;
          a[kSweepQ * m + 2] = a[kSweepQ * m + 2] + x;
          a[kSweepQ * m + 3] = a[kSweepQ * m + 3] + y;
          a[kSweepQ * m + 4] = a[kSweepQ * m + 4] + z;
        }
        double s[kMaxQ];
        for (int q = 0; q <= kSweepQ * K; q++) s[q] = (double)a[q];
        for (int j = 0; j < K; j++) s[kSweepQ * j] = (double)cnt[j];
        if (pt_sweep_update<H>(S, K, s, l)) break;
      }
    }
    double s1[kMaxQ];
    {
      H zs[kMaxCluster] = {}, cx = 0, cy = 0, cz = 0, sz = 0, sq = 0;
      for (int i = 0; i < n; i++) {
        if (S.clustered) zs[ncl[i]] = zs[ncl[i]] + zl[i];
        H x, y, z;
        pt_cart<H>(pt_roundtrip<H>(xl[i], S.clustered), pt_roundtrip<H>(yl[i], S.clustered), x, y, z);
        cx = cx + x; cy = cy + y; cz = cz + z;
        sz = sz + zl[i]; sq = sq + zl[i] * zl[i];
      }
      for (int j = 0; j < K; j++) s1[j] = (double)zs[j];
      const double t[kFinal1Q] = {(double)s_topo, (double)s_hmix, (double)s_pv, (double)s_tropo, (double)c_hmix, (double)c_pv, (double)c_tropo,
                                  (double)cx, (double)cy, (double)cz, (double)sz, (double)sq};
      for (int q = 0; q < kFinal1Q; q++) s1[K + q] = t[q];
    }
    pt_final1_update<H>(S, K, s1);
    {
      const double dpr = pt_dpr<H>();
      const double slat2 = pt_sin((double)S.val[1] / dpr), clat2 = pt_cos((double)S.val[1] / dpr);
      H zr = 0, rd = 0;
      for (int i = 0; i < n; i++) {
        if (S.clustered) { const H zd = zl[i] - S.zclust[ncl[i]]; zr = zr + zd * zd; }
        const H dist = pt_distance<H>(pt_roundtrip<H>(yl[i], S.clustered), pt_roundtrip<H>(xl[i], S.clustered), S.val[1], S.val[0], slat2, clat2);
        rd = rd + dist * dist;
      }
      const double s2[2] = {(double)zr, (double)rd};
      pt_final2_update<H>(S, K, s2);
    }
    fputs(pt_record<H>(h[0], h[1], S.val).c_str(), stdout);
    printf("# %d", S.iterations);
    for (int j = 0; j < K; j++) printf(" %d", S.clustered ? S.numb[j] : 0);
    printf("\n");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> h = get<int32_t>(f, 3);
  if (h[1] != 5) { fprintf(stderr, "plumetraj_host: the record has five clusters\n"); return 2; }
  return h[0] == 4 ? run<float>(f, h[1], h[2]) : run<double>(f, h[1], h[2]);
}
