"""Sensitivity to initial conditions (initial_cond_calc.f90, initial_cond_output.f90; fpx_config.device_initcond = 1):
fpx_initcond_finish, fpx_get_initcond, fpx_initial_cond_output, fpx_initcond_time.

CPU: the numpy restatement tests/initcond_ref.py against what flang builds of the unmodified routines produce
(tests/golden/ic_r4.npz, ic_r8.npz: init_cond bit for bit, the grid_initial files byte for byte), the host-compiled
per-particle body of fpx_initcond.hpp against the same fixtures bit for bit (the exact pin of the device arithmetic), the
coverage of the synthetic cases, and -- where flang and the reference are present -- a fresh build.
GPU: the kernels against the restatement applied to the particles downloaded before and after each step.  The terms are
the reference's, bit for bit (pinned above); the device adds them with atomics in another order than the serial loop, so
a cell that received m terms may differ from the serial sum ref by at most 2 m u ref (u = 2^-24 / 2^-53): the bound for
two summation orders of the same m non-negative terms (each order errs by at most (m - 1) u times the sum, to first
order).  Cells with one term are bit-equal, cells with none exactly zero."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import initcond_ref as ir
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ("r4", "r8")
sys.path.insert(0, GOLD)


# ---- CPU ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated():
    """(init_cond, stats, files, runs) of the restatement per (kind, variant): computed once, never modified."""
    out = {}
    for kind in KINDS:
        for v in syn.IC_VARIANTS:
            c = syn.initcond_case(v)
            st, runs = {}, {}
            grid = ir.run_case(c, kind, st)
            grid.setflags(write=False)
            files = ir.initial_cond_output(grid, kind, c["itime"], c["xmass"], c["ind_rel"], c["rho_rel"], runs)
            out[kind, v] = (grid, st, files, runs)
    return out


@pytest.mark.parametrize("variant", syn.IC_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(restated, kind, variant):
    """init_cond after the serial loop bit for bit, the files of initial_cond_output byte for byte, in both real kinds."""
    gold = np.load(os.path.join(GOLD, f"ic_{kind}.npz"))
    grid, _, files, _ = restated[kind, variant]
    ref = gold[f"init_cond_{variant}"]
    assert grid.dtype == ref.dtype == ir.RT[kind] and grid.shape == ref.shape
    assert np.array_equal(grid, ref)
    assert np.count_nonzero(ref) > 50
    for ks, data in enumerate(files):
        assert data == gold[f"file_{variant}_{ks + 1}"].tobytes(), ks
    assert len(files) == int(syn.initcond_case(variant)["nspec"])


HOST_MAIN = textwrap.dedent(r"""
    // the per-particle body of fpx_initcond.hpp as host code, run serially in particle order over the input file of
    // tests/golden/ref_ic_driver.f90; writes init_cond as f8
    #define FPX_IC_HOST
    #include "fpx_initcond.hpp"
    #include <cstdint>
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <vector>
    template <typename T> static std::vector<T> rd(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); } return v; }
    template <typename H> struct HostRho {
      const H *r; int nx, ny;
      H operator()(int ix, int jy, int ind) const { return r[(size_t)ix + (size_t)nx * ((size_t)jy + (size_t)ny * (size_t)(ind - 1))]; }
    };
    template <typename H> static int run(const char *fin, const char *fout) {
      FILE *f = fopen(fin, "rb");
      if (!f) return 1;
      const std::vector<int32_t> hi = rd<int32_t>(f, 16);
      const int nx = hi[0], ny = hi[1], nz = hi[2], n = hi[3], nxg = hi[4], nyg = hi[5], nzg = hi[6], ns = hi[7], mps = hi[8];
      const std::vector<double> hg = rd<double>(f, 8), height8 = rd<double>(f, nz), outh8 = rd<double>(f, nzg);
      const std::vector<double> rho1 = rd<double>(f, (size_t)nx * ny * nz), rho2 = rd<double>(f, (size_t)nx * ny * nz);
      rd<double>(f, (size_t)mps * ns); rd<double>(f, mps);
      const std::vector<double> xt = rd<double>(f, n), yt = rd<double>(f, n), zt = rd<double>(f, n), xm = rd<double>(f, (size_t)n * ns);
      const std::vector<int32_t> npoint = rd<int32_t>(f, n), itra1 = rd<int32_t>(f, n);
      fclose(f);
      const std::vector<double> &rsel = hi[15] == 1 ? rho1 : rho2;      // memind(2)
      std::vector<H> height(height8.begin(), height8.end()), outh(outh8.begin(), outh8.end()), rho(rsel.begin(), rsel.end()), mass(xm.begin(), xm.end());
      std::vector<H> grid((size_t)nxg * nyg * nzg * ns * mps, (H)0);
      fpx::ic::Args<H> A;
      A.linit_cond = hi[11]; A.nx = nx; A.ny = ny; A.nz = nz;
      A.numxgrid = nxg; A.numygrid = nyg; A.numzgrid = nzg; A.nspec = ns; A.maxpointspec_act = mps;
      A.use_npoint = hi[9] == 1 && hi[10] == 0;
      A.dx = (H)hg[0]; A.dy = (H)hg[1]; A.dxout = (H)hg[4]; A.dyout = (H)hg[5];
      A.xoutshift = (H)hg[2] - (H)hg[6]; A.youtshift = (H)hg[3] - (H)hg[7];
      A.outheight = outh.data(); A.init_cond = grid.data();
      const HostRho<H> R{rho.data(), nx, ny};
      for (int j = 0; j < n; j++) {
        if (itra1[j] != hi[13]) continue;                               // initial_cond_calc.f90:37
        fpx::ic::ic_particle<H>(A, height.data(), R, xt[j], yt[j], (H)zt[j], npoint[j], mass.data() + j, (size_t)n);
      }
      std::vector<double> o(grid.begin(), grid.end());
      f = fopen(fout, "wb");
      if (!f || fwrite(o.data(), 8, o.size(), f) != o.size()) return 1;
      return fclose(f);
    }
    int main(int argc, char **argv) {
      if (argc < 4) return 1;
      return strcmp(argv[1], "r4") == 0 ? run<float>(argv[2], argv[3]) : run<double>(argv[2], argv[3]);
    }
""")


@pytest.fixture(scope="module")
def host_body(tmp_path_factory):
    d = tmp_path_factory.mktemp("ic_host")
    src, exe = d / "ic_host.cpp", d / "ic_host"
    src.write_text(HOST_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "flexpart_amd", "csrc"),
                           str(src), "-o", str(exe)])
    return str(exe), d


@pytest.mark.parametrize("variant", syn.IC_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_compiled_device_body_reproduces_the_reference(host_body, kind, variant):
    """ic_locate / ic_value / ic_particle of fpx_initcond.hpp, compiled as host code and run serially in particle order,
    give the reference's init_cond bit for bit: the device's terms and cell decisions are the reference's."""
    import make_initcond_golden as mk
    exe, d = host_body
    c = syn.initcond_case(variant)
    fin, fout = str(d / f"in_{kind}_{variant}.bin"), str(d / f"out_{kind}_{variant}.bin")
    mk.write_input(c, fin)
    subprocess.check_call([exe, kind, fin, fout])
    ref = np.load(os.path.join(GOLD, f"ic_{kind}.npz"))[f"init_cond_{variant}"]
    got = np.fromfile(fout, np.float64).reshape(ref.shape)
    assert np.array_equal(got, ref.astype(np.float64))
    assert np.count_nonzero(got) > 50


@pytest.mark.parametrize("kind", KINDS)
def test_cases_cover_every_branch(restated, kind):
    """Everything the routines can do appears in the fixtures, counted by the restatement while it runs."""
    for v in syn.IC_VARIANTS:
        _, st, _, runs = restated[kind, v]
        for key in ("direct_west", "direct_south", "direct_east", "direct_north",          # direct attribution on each border
                    "kernel_ixp_plus", "kernel_ixp_minus", "kernel_jyp_plus", "kernel_jyp_minus",
                    "neighbour_out_west", "neighbour_out_south",                         # ixp = -1, jyp = -1 (xl = 0.5, yl = 0.5)
                    "xl_negative", "yl_negative", "above_top", "not_due"):
            assert st[key] > 0, (v, key, st)
        # beyond numxgrid - 1.5 / numygrid - 1.5 the direct attribution takes over: the kernel never looks east or north of the grid
        assert st["neighbour_out_east"] == 0 and st["neighbour_out_north"] == 0
        assert st["guarded"] == 0                                                         # no particle needs the engine's guards
        assert all(r >= 2 for r in runs.values()), (v, runs)                              # zero runs and the alternating sign
    assert restated[kind, "points"][1]["kp_gt_1"] > 0
    grid = restated[kind, "points"][0]
    assert all(np.count_nonzero(grid[kp, ks]) > 0 for kp in range(3) for ks in range(2))
    # mdomainfill = 1: nrelpointer = 1 although npoint is the particle number
    assert restated[kind, "domainfill"][1]["kp_gt_1"] == 0 and int(syn.initcond_case("domainfill")["npoint"].max()) > 3
    # the two units differ by the air density only
    assert not np.array_equal(restated[kind, "mass"][0], restated[kind, "mixing"][0])
    assert np.array_equal(restated[kind, "mass"][0] != 0, restated[kind, "mixing"][0] != 0)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_a_live_build_of_the_reference(kind, tmp_path):
    import make_initcond_golden as mk
    if not mk.available():
        pytest.skip("flang or the reference tree is not present")
    exe = mk.build(kind, str(tmp_path))
    for v in syn.IC_VARIANTS:
        c = syn.initcond_case(v)
        grid, files = mk.run(exe, c, str(tmp_path))
        mine = ir.run_case(c, kind)
        assert np.array_equal(mine.astype(np.float64), grid), v
        assert ir.initial_cond_output(mine, kind, c["itime"], c["xmass"], c["ind_rel"], c["rho_rel"]) == files, v


def test_header_cites_the_reference_lines():
    """The public header names the new entry points next to the reference lines they replace."""
    text = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    for name in ("fpx_initcond_finish", "fpx_get_initcond", "fpx_initial_cond_output", "fpx_initcond_time", "fpx_initout", "device_initcond",
                 "unless device_initcond = 1", "timemanager.f90:631", "timemanager.f90:702", "timemanager.f90:735-737", "timemanager.f90:745",
                 "initial_cond_calc.f90:37-197", "initial_cond_output.f90:58-130", "linversionout"):
        assert name in text, name


def test_struct_sizes_and_abi(tmp_path):
    """device_initcond took the last reserved integer of fpx_config: its size is the C compiler's and unchanged."""
    from flexpart_amd import _lib
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flexpart_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(fpx_config), offsetof(fpx_config, device_initcond), offsetof(fpx_config, device_partavg), sizeof(fpx_initout));\n  return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, off_pa, size_io = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_lib.FpxConfig) and off == _lib.FpxConfig.device_initcond.offset == off_pa + 4
    assert off + 4 == size                                               # the last field: nothing is reserved any more
    assert size_io == C.sizeof(_lib.FpxInitout) == 16
    assert not hasattr(_lib.FpxConfig, "reserved")
    lib = _lib.load()
    assert lib.fpx_abi_version() == 4
    for name in ("fpx_initcond_finish", "fpx_get_initcond", "fpx_initial_cond_output", "fpx_initcond_time"):
        assert name in _lib.SYMBOLS and getattr(lib, name)


# ---- GPU ------------------------------------------------------------------------------------------------------

ENGINES = [(8, 8), (4, 4)]          # (compute_real_bytes, host_real_bytes): fp64 engine with an r8 host, f32 engine with an r4 host
NSTEPS = 3


def ic_scenario(linit_cond=2, device_initcond=1, quiet=False):
    """Backward variant of syn.small(n=1500, nx=20, ny=12, nz=10) on a limited-area one-degree grid, two decaying species,
    three release points with ioutputforeachrelease = 1.  The cloud is drawn together over met x 0 .. 2.2, y 3.8 .. 6.2 at
    the western boundary, which the backward run's mean wind carries it across; the output grid of 12 x 8 x 3 quarter cells
    starts one met cell WEST of the domain (xl = 4 xt + 4), so a particle that has just left it still lies over the
    grid.  Release times are spread over 5000 s with lage = (1800, 5400): every step some particles get too old.  Every
    ninth particle carries 1.03e-4 of its nominal mass, just above minmass, and the decay takes it below within two steps.
    quiet: the cloud sits in the middle of the domain under an output grid there, nothing gets old, every third particle
    is below minmass from the start -- the only terminations are the ones for small mass."""
    nx, ny = 20, 12
    sc = syn.small(n=1500, nx=nx, ny=ny, nz=10, nsteps=NSTEPS, nspec=2, global_grid=False, ldirect=-1)
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    x0, y0 = (6.0, 3.0) if quiet else (0.0, 3.8)
    sc["xtra1"] = x0 + (6.0 if quiet else 2.2) * np.asarray(sc["xtra1"]) / float(nx - 1)
    sc["ytra1"] = y0 + (4.0 if quiet else 2.4) * np.asarray(sc["ytra1"]) / float(ny - 1)
    syn.add_outgrid(sc, 12, 8, 3, dxout=dx / 4.0, dyout=dy / 4.0, outlon0=xlon0 + (7.5 if quiet else -1.0) * dx, outlat0=ylat0 + 4.0 * dy, old_fraction=0.0)
    if quiet:
        syn.add_release_points(sc, xmass=[[1.0, 1.0, 1.0]] * 2, npart_rel=[500, 500, 500], tiny_every=3)
    else:
        syn.add_release_points(sc, xmass=[[1.0, 2.0, 0.5], [3.0, 1.0, 1.5]], npart_rel=[500, 500, 500], lage=[1800, 5400], max_age=5000,
                               near_every=9)
        sc["decay"] = np.array([3.0e-5, 2.5e-5])
    sc.update(linit_cond=linit_cond, device_initcond=device_initcond)
    return sc


def kind_of(hb):
    return "r4" if hb == 4 else "r8"


def make_engine(sc, cb, hb, **kw):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    return Engine(sc, compute_real_bytes=cb, host_real_bytes=hb, rng_mode=RNG_PHILOX, seed=4711, **kw)


def contributors(sc, cb, itime, before, after):
    """The call-site rules of timemanager.f90:630-632,681,701-703 applied to two downloads around a step at `itime`:
    (left the domain, terminated for small mass, terminated for age) as masks over the particles."""
    rt = np.float64 if cb == 8 else np.float32                          # the engine's arithmetic type
    nx, ny = int(sc["grid"][0]), int(sc["grid"][1])
    gone = (before["itra1"] == itime) & (after["itra1"] == syn.DEAD)
    x, y = after["xtra1"], after["ytra1"]
    left = gone & (~(x >= 0.0) | ~(x < float(nx - 1)) | ~(y >= 0.0) | ~(y <= float(ny - 1)))
    kp = np.clip(after["npoint"], 1, int(sc["numpoint"])) - 1
    xmr = np.asarray(sc["xmass"], np.float64).astype(rt)[:, kp]          # xmass(npoint(j),ks)
    npart = np.asarray(sc["npart_rel"])[kp].astype(rt)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(xmr > 0, (npart[None, :] * after["xmass1"].astype(rt)).astype(rt) / xmr, rt(0.0)).astype(rt)
    small = gone & ~left & (frac.max(axis=0) < rt(0.0001))
    return left, small, gone & ~left & ~small


def stepped(sc, cb, hb, nsteps=NSTEPS, finish=True, **kw):
    """nsteps steps and the finish: (engine, fetched grid, serial reference, terms per cell, summed step statistics)."""
    P = ir.params_from_scenario(sc, kind_of(hb))
    eng = make_engine(sc, cb, hb, **kw)
    ref, cnt = P.new_grid(), np.zeros(P.new_grid().shape, np.int64)
    tot = dict(n_left_domain=0, n_min_mass=0, n_max_age=0, case1=0, case2=0, case3=0, case1_adding=0)
    before = eng.download()
    for _ in range(nsteps):
        itime = eng.itime
        stats = eng.step()
        after = eng.download()
        for k in ("n_left_domain", "n_min_mass", "n_max_age"):
            tot[k] += int(stats[k])
        left, small, old = contributors(sc, cb, itime, before, after)
        tot["case1"] += int(left.sum()); tot["case2"] += int(small.sum()); tot["case3"] += int(old.sum())
        tot["case1_adding"] += int(ir.locate(P, after["xtra1"][left], after["ytra1"][left], after["ztra1"][left], after["npoint"][left])["adds"].sum())
        # :631 sees the masses from before the step, :702 the ones after deposition and decay
        mass = np.where(left[None, :], before["xmass1"], after["xmass1"])
        fake = np.where(left | old, itime, itime + 1)
        ir.initial_cond_calc(ref, P, itime, after["xtra1"], after["ytra1"], after["ztra1"], mass, after["npoint"], fake, count=cnt)
        before = after
    if finish:
        eng.initcond_finish(eng.itime)                                  # timemanager.f90:735-737
        ir.initial_cond_calc(ref, P, eng.itime, before["xtra1"], before["ytra1"], before["ztra1"], before["xmass1"], before["npoint"],
                             before["itra1"], count=cnt)
    return eng, eng.get_initcond(), ref, cnt, tot


def check_grid(got, ref, cnt, hb):
    u = 2.0 ** -24 if hb == 4 else 2.0 ** -53
    assert got.dtype == ref.dtype and got.shape == ref.shape
    g, r = got.astype(np.float64), ref.astype(np.float64)
    err = np.abs(g - r)
    bound = 2.0 * cnt * u * r
    worst = float(np.max(np.where(cnt > 1, err / np.where(bound > 0, bound, 1.0), 0.0)))
    print(f"cells set {np.count_nonzero(r)}, with one term {int((cnt == 1).sum())}, most terms {int(cnt.max())}, worst error / bound {worst:.3f}")
    assert np.all(got[cnt == 0] == 0)
    assert np.array_equal(got[cnt == 1], ref[cnt == 1])
    assert np.all(r >= 0) and np.all(err <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize("linit_cond", [1, 2])
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_step_parity(built, cb, hb, linit_cond):
    """init_cond after 3 steps and fpx_initcond_finish against the serial restatement over the downloads, with the three
    kinds of termination present.  Fails on an engine without the feature: it refuses the configuration."""
    sc = ic_scenario(linit_cond)
    eng, got, ref, cnt, tot = stepped(sc, cb, hb)
    eng.close()
    print(tot)
    assert tot["n_left_domain"] > 0 and tot["n_min_mass"] > 0 and tot["n_max_age"] > 0
    assert (tot["case1"], tot["case2"], tot["case3"]) == (tot["n_left_domain"], tot["n_min_mass"], tot["n_max_age"])
    # mass unit: a particle outside the met grid has no air density and adds nothing (the engine's guard); mixing ratio: it does
    assert (tot["case1_adding"] > 0) == (linit_cond == 2)
    check_grid(got, ref, cnt, hb)
    assert np.count_nonzero(got) > 50 and cnt.max() >= 8
    assert all(np.count_nonzero(got[kp, ks]) > 0 for kp in range(3) for ks in range(2))


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_terminations_before_the_finish(built, cb, hb):
    """Without the finish the grid holds only what the step's own calls added: the particles that left the domain (with
    the masses from before the step; linit_cond = 2, the grid reaches beyond the domain) and the ones that got too old."""
    sc = ic_scenario(2)
    eng, got, ref, cnt, tot = stepped(sc, cb, hb, finish=False)
    eng.close()
    check_grid(got, ref, cnt, hb)
    assert np.count_nonzero(got) > 20 and tot["case1_adding"] > 0 and tot["case3"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_small_mass_terminations_contribute_nothing(built, cb, hb):
    """timemanager.f90:681 comes before :701: a particle terminated for small mass never reaches the call."""
    sc = ic_scenario(2, quiet=True)
    eng, got, ref, cnt, tot = stepped(sc, cb, hb, finish=False)
    assert tot["n_min_mass"] > 100 and tot["n_left_domain"] == 0 and tot["n_max_age"] == 0
    assert np.count_nonzero(got) == 0 and np.count_nonzero(ref) == 0
    eng.initcond_finish()
    assert np.count_nonzero(eng.get_initcond()) > 50
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_trajectories_are_untouched(built, cb, hb):
    res = []
    for on in (1, 0):
        eng = make_engine(ic_scenario(2 * on, device_initcond=on), cb, hb)
        for _ in range(NSTEPS):
            eng.step()
        res.append(eng.download())
        eng.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k
    assert (res[0]["itra1"] == syn.DEAD).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_sorted_cloud_gives_the_same_grid(built, cb, hb):
    eng, got, ref, cnt, _ = stepped(ic_scenario(1), cb, hb, sort_interval=1)
    eng.close()
    check_grid(got, ref, cnt, hb)
    assert np.count_nonzero(got) > 50


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_initial_cond_output_files(built, tmp_path, cb, hb):
    """fpx_initial_cond_output writes, byte for byte, what the restatement's writer makes of the fetched grid; the grid
    stays as it is."""
    kind = kind_of(hb)
    sc = ic_scenario(1)
    eng = make_engine(sc, cb, hb)
    for _ in range(NSTEPS):
        eng.step()
    eng.initcond_finish()
    grid = eng.get_initcond()
    rho_rel = np.array([1.125, 0.9375, 1.0625])
    prefix = str(tmp_path) + os.sep
    names = eng.initial_cond_output(eng.itime, prefix, ind_rel=1, rho_rel=rho_rel)
    after = eng.get_initcond()
    runs = {}
    want = ir.initial_cond_output(grid, kind, eng.itime, sc["xmass"], 1, rho_rel, runs)
    assert [os.path.basename(n) for n in names] == ["grid_initial_001", "grid_initial_002"] == sorted(os.listdir(tmp_path))
    for name, data in zip(names, want):
        assert open(name, "rb").read() == data
    assert min(runs.values()) >= 2 and np.array_equal(after, grid)
    for f in names:
        os.remove(f)
    eng.initial_cond_output(eng.itime, prefix)                           # ind_rel = 0: fact_recept = 1, no rho_rel
    assert [open(n, "rb").read() for n in names] == ir.initial_cond_output(grid, kind, eng.itime, sc["xmass"])
    eng.close()


@pytest.mark.gpu
def test_states_and_refusals(built):
    from flexpart_amd.engine import Engine, _vp
    sc = syn.small(n=10, nx=20, ny=12, nz=10, nsteps=1, ldirect=-1)
    out = np.zeros(16, np.float64)
    sc["linit_cond"] = 1
    with pytest.raises(Exception, match="linit_cond >= 1: the particle loop's initial_cond_calc .timemanager.f90:631,702. is not computed by this engine") as e:
        Engine(sc)                                           # linit_cond alone: refused as before, same status, same text
    assert e.value.code == -5                                # FPX_ERR_UNSUPPORTED
    sc["device_initcond"] = 1
    eng = Engine(sc)                                         # accepted; no output grid yet
    with pytest.raises(Exception, match="fpx_outgrid_init") as e:
        eng.step()
    assert e.value.code == -3                                # FPX_ERR_STATE
    assert eng.lib.fpx_get_initcond(eng.h, _vp(out), 0, 0) == -3
    assert eng.lib.fpx_initcond_finish(eng.h, 0) == -3
    eng.close()
    for bad in (dict(linit_cond=0), dict(linit_cond=3), dict(device_initcond=2)):
        with pytest.raises(Exception) as e:
            Engine(dict(sc, **bad))
        assert e.value.code == -1, bad                       # FPX_ERR_ARG
    fw = syn.small(n=10, nx=20, ny=12, nz=10, nsteps=1)
    fw.update(linit_cond=1, device_initcond=1)
    with pytest.raises(Exception, match="ldirect = 1") as e:
        Engine(fw)
    assert e.value.code == -1
    fw.update(linit_cond=0, device_initcond=0)
    eng = Engine(fw)
    assert eng.lib.fpx_initcond_finish(eng.h, 0) == -3       # an engine without the switch
    assert eng.lib.fpx_get_initcond(eng.h, _vp(out), 0, 0) == -3
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_checkpoint_carries_the_grid(built, tmp_path, cb, hb):
    """The grid fetched after checkpoint_read is the one fetched before checkpoint_write, bit for bit; a file of one kind is
    refused by an engine of the other; without the switch the file has the length it always had."""
    sc = ic_scenario(2)
    eng = make_engine(sc, cb, hb)
    for _ in range(2):
        eng.step()
    want = eng.get_initcond()
    path = str(tmp_path / "ck.bin")
    eng.checkpoint_write(path)
    eng.close()
    eng = make_engine(sc, cb, hb)
    assert np.count_nonzero(eng.get_initcond()) == 0
    eng.checkpoint_read(path)
    got = eng.get_initcond()
    eng.close()
    assert np.array_equal(got, want) and np.count_nonzero(want) > 20
    off = ic_scenario(0, device_initcond=0)
    eng = make_engine(off, cb, hb)
    with pytest.raises(Exception, match="device_initcond"):
        eng.checkpoint_read(path)
    for _ in range(2):
        eng.step()
    plain = str(tmp_path / "plain.bin")
    eng.checkpoint_write(plain)
    eng.close()
    eng = make_engine(sc, cb, hb)
    with pytest.raises(Exception, match="device_initcond"):
        eng.checkpoint_read(plain)
    eng.close()
    assert os.path.getsize(path) - os.path.getsize(plain) == 8 + want.size * hb
    for file, flag in ((plain, 0), (path, 4)):
        raw = open(file, "rb").read(192)
        assert np.frombuffer(raw[60:64], np.int32)[0] == flag
        numpart = int(np.frombuffer(raw[24:32], np.int64)[0])
        g3, g2, g3n, g2n, nrec, rng_bytes, cbase = (int(v) for v in np.frombuffer(raw[64:120], np.uint64))
        assert (numpart, g3n, g2n, nrec, cbase) == (1500, 0, 0, 0, 0)
        per_particle = 2 * 8 + 7 * cb + 6 * 4 + 2 + 2 * cb             # as tests/test_calcfluxes.py has it, with two species
        base = 192 + rng_bytes + numpart * per_particle + g3 * cb + 2 * g2 * 4
        assert int(np.frombuffer(raw[184:192], np.uint64)[0]) == os.path.getsize(file) == base + (flag != 0) * (8 + want.size * hb)


@pytest.mark.gpu
def test_initcond_time(built):
    """fpx_initcond_time: one launch per step and a positive device time; reset starts over."""
    eng = make_engine(ic_scenario(2), 8, 8)
    for _ in range(NSTEPS):
        eng.step()
    ms, launches = eng.initcond_time(reset=True)
    assert launches == NSTEPS and ms > 0
    assert eng.initcond_time() == (0.0, 0)
    eng.step()
    assert eng.initcond_time()[1] == 1
    eng.close()
