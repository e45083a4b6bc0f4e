"""getvdep on the device (calcpar.f90:171-189): the dry-deposition velocities from ustar, oli, the surface analysis and
the host's land-use and resistance tables.

Unlike calcpar.f90 itself the whole chain -- getvdep.f90, getrb.f90, getrc.f90, raerod.f90, psih.f90, partdep.f90,
caldate.f90, ew.f90 -- compiles with flang in both real kinds, so this row is pinned to the reference itself: the fixtures
tests/golden/gv_r4.npz, gv_r8.npz hold what the unmodified routines return (tests/golden/make_getvdep_golden.py with our
driver ref_gv_driver.f90) for the synthetic case of tests/getvdep_ref.py, and both the numpy restatement and the device
kernel are compared with them directly.

Tolerances: 1e-10 (r8) and 2e-4 (r4) of the largest value of the species, the device-to-restatement tolerances of
tests/test_calcpar.py (the libm of numpy, of flang's runtime and of the device need not agree to the bit in x**y).  Two
decisions of the chain are discrete in a computed quantity: rh > 0.9 (getrc.f90:60,90) and alpha <= log10(eps)
(partdep.f90:81).  A column within rounding reach of one of them (relative distance 1e-9 in r8, 1e-4 in r4, the reach
tests/test_calcpar.py uses) may take the other branch; such columns are counted and capped, never masked out silently.

The case has three wind-field times, not two: a winter date (lseason 4) is always met by summer (1) half a year on in
the other hemisphere (getvdep.f90:54-56), so two times give at most four of the five seasonal categories."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import getvdep_ref as gr
from flexpart_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"r8": 1e-10, "r4": 2e-4}
REACH = {"r8": 1e-9, "r4": 1e-4}
NT = len(syn.GV_WFTIMES)
GIVEN = ("ustar", "oli", "ps", "tt2", "td2")

_cache = {}


def restated(kind, t):
    """The restatement of fixture time t, computed once and shared."""
    if (kind, t) not in _cache:
        tables, gin = gr.fixture_case(t)
        _cache[(kind, t)] = gr.getvdep_ref(tables, gin, gr.DY, gr.YLAT0, kind)
    return _cache[(kind, t)]


def fragile(kind, r):
    return (r["margin_rh"] < REACH[kind]) | (r["margin_alpha"] < REACH[kind])


def maker():
    spec = importlib.util.spec_from_file_location("make_getvdep_golden", os.path.join(GOLD, "make_getvdep_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def worst(got, gold):
    """max over the species of max|got - gold| / max|gold|, per column [ny][nx]"""
    scale = np.abs(gold).reshape(gold.shape[0], -1).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)[:, None, None]
    return (np.abs(got - gold) / scale).max(axis=0)


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_restatement_matches_reference_fixtures(kind):
    """tests/getvdep_ref.py against the flang build of the unmodified routines, every species and column of the three
    wind-field times.  Observed maximum: 2.5e-16 (r8), 2.2e-7 (r4) of the species' largest value."""
    gold = np.load(os.path.join(GOLD, f"gv_{kind}.npz"))
    seen = 0.0
    for t in range(NT):
        tables, gin = gr.fixture_case(t)
        for k in gr.FIELDS:                      # the fixture's inputs are the ones regenerated here, bit for bit
            assert np.array_equal(gold[f"{k}{t}"], gin[k]), k
        assert int(gold[f"wftime{t}"]) == gin["wftime"]
        for k in gr.TABLES:
            assert np.array_equal(gold[k], tables[k]), k
        r = restated(kind, t)
        w = worst(r["vdep"], gold[f"vdep{t}"])
        seen = max(seen, float(w.max()))
        print(f"getvdep restatement vs flang fixture {kind} t={t}: max relative deviation {w.max():.3e}")
        assert w.max() <= TOL[kind], (t, float(w.max()))
        assert np.all(gold[f"vdep{t}"][3] == 0.0) and np.all(gold[f"vdep{t}"][2] == tables["dryvel"][2].astype(np.float32 if kind == "r4" else np.float64))
    print(f"getvdep restatement vs flang fixture {kind}: max over all times {seen:.3e}")


@pytest.mark.ref
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_restatement_matches_live_reference(kind):
    """The same against the reference compiled on the spot, for another draw of the inputs."""
    mk = maker()
    if not mk.available():
        pytest.skip("reference sources and flang not present")
    bd = os.path.join(ROOT, "oracle", "_ref", "gvref")
    os.makedirs(bd, exist_ok=True)
    exe = mk.build(kind, bd, modules_from=os.path.join(ROOT, "oracle", "_ref", f"obj_{kind}"))
    tables = syn.getvdep_tables(gr.NX, gr.NY, gr.NSPEC)
    gin = syn.getvdep_inputs((gr.NY, gr.NX), seed=977, wftime=syn.GV_WFTIMES[1])
    live = mk.run(exe, tables, gin, gr.DY, gr.YLAT0, bd)
    r = gr.getvdep_ref(tables, gin, gr.DY, gr.YLAT0, kind)
    ok = ~fragile(kind, r)
    w = worst(r["vdep"], live)
    assert w[ok].max() <= TOL[kind], float(w[ok].max())
    assert (~ok).mean() <= (0.0 if kind == "r8" else 0.005)
    t, g0 = gr.fixture_case(0)
    gold = np.load(os.path.join(GOLD, f"gv_{kind}.npz"))
    assert np.array_equal(mk.run(exe, t, g0, gr.DY, gr.YLAT0, bd), gold["vdep0"])     # the committed fixture is what the reference gives


def test_fixture_covers_every_branch_with_margin():
    """Every branch of the chain occurs in the fixture's own inputs, and none of its columns sits on a threshold."""
    seasons = set()
    for t in range(NT):
        tables, gin = gr.fixture_case(t)
        r8, r4 = restated("r8", t), restated("r4", t)
        seasons |= set(int(v) for v in r8["lseason"])
        assert np.array_equal(r8["lseason"], r4["lseason"])
        snow, rr, rh, tc = np.asarray(gin["sd"]), r8["rr"], r8["rh"], r8["tc"]
        L = 1.0 / np.asarray(gin["oli"])
        xl = np.asarray(tables["xlanduse"])
        n = {"snow": int((snow > 0.001).sum()), "no snow": int((snow <= 0.001).sum()), "rain": int((rr > 0).sum()),
             "dew without rain": int(((rh > 0.9) & ~(rr > 0)).sum()), "dry": int(((rh <= 0.9) & ~(rr > 0)).sum()),
             "frost": int((tc <= 0).sum()), "heat": int((tc >= 40).sum()), "stomata open": int(((tc > 0) & (tc < 40)).sum()),
             "stable": int((L > 0).sum()), "unstable": int((L < 0).sum()), "L = 9999": int((L == 9999.0).sum()), "L = -9999": int((L == -9999.0).sum()),
             "calm": int((np.asarray(gin["ustar"]) == 1e-8).sum()), "absent classes": int((xl == 0).sum()), "present classes": int((xl > 1e-5).sum())}
        # both sides of the alpha switch (partdep.f90:81), recomputed here from the inputs in double
        pa, temp, ust = (np.asarray(gin[k]) for k in ("ps", "tt2", "ustar"))
        myl = np.where(tc < 0, 1.718 + 0.0049 * tc - 1.2e-5 * tc * tc, 1.718 + 0.0049 * tc) * 1e-5
        nyl = myl / (pa / (287.0 * temp))
        vs = np.asarray(tables["vset"])[:, 1]
        alpha = -3.0 / (vs[:, None, None] / 9.81 * ust[None] ** 2 / nyl[None])
        moving = ust[None] > 1e-5
        n["alpha below"] = int(((alpha <= -5.0) & moving).sum())
        n["alpha above"] = int(((alpha > -5.0) & moving).sum())
        print(f"getvdep fixture t={t}: {n}")
        assert all(v >= 5 for v in n.values()), n
        for kind, r in (("r8", r8), ("r4", r4)):
            frac = float(fragile(kind, r).mean())
            print(f"getvdep fixture t={t} {kind}: share of columns within {REACH[kind]:g} of a threshold {frac:.5f}")
            assert frac <= (0.0 if kind == "r8" else 0.005), (t, kind, frac)
    assert seasons == {1, 2, 3, 4, 5}, seasons


def test_new_structs_have_the_size_the_c_compiler_gives_them(tmp_path):
    import subprocess
    from flexpart_amd import _lib
    pairs = [("fpx_getvdep_tables", _lib.FpxGetvdepTables), ("fpx_getvdep_in", _lib.FpxGetvdepIn), ("fpx_calcpar_in", _lib.FpxCalcparIn)]
    src = tmp_path / "sizes.c"
    src.write_text('#include "flexpart_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n, _ in pairs)
                   + '  printf("device_vdep %zu\\n", offsetof(fpx_calcpar_in, device_vdep));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n, t in pairs:
        assert int(got[n]) == C.sizeof(t), (n, got[n], C.sizeof(t))
    assert C.sizeof(_lib.FpxCalcparIn) == 6 * 8 + 4 * 4                    # unchanged: device_vdep took the first reserved integer
    assert int(got["device_vdep"]) == _lib.FpxCalcparIn.device_vdep.offset == 6 * 8 + 4


def test_abi_version_is_unchanged(built):
    from flexpart_amd import _lib
    assert _lib.load().fpx_abi_version() == 4


# ---- GPU ---------------------------------------------------------------------------------------------------------
def scenario(nx, ny, nz, nspec, geom, drydep=1, **extra):
    """A run without particles and without fields: grid, switches and the species of a DRYDEP run."""
    sc = dict(grid=np.array([nx, ny, nz], np.int32), geom=np.asarray(geom, np.float64), globalflags=np.zeros(3, np.int32), nspec=nspec, npart=0)
    skip = ("uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep") + tuple(extra.pop("skip", ()))
    sc.update({k: v for k, v in syn.base_scenario(8, 6, nz, nspec=nspec).items() if k not in sc and k not in skip})
    sc.update(drydep=drydep, drydepspec=np.full(nspec, drydep, np.int32))
    sc.update(extra)
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_device_matches_the_reference_fixture(built, kind):
    """fpx_getvdep_init + fpx_getvdep with all of ustar, oli, ps, tt2, td2 given, against what flang's build of the
    unmodified routines returned: the three wind-field times, each into slot 1 and slot 2, arrays padded to 40 x 32."""
    from flexpart_amd.engine import Engine
    gold = np.load(os.path.join(GOLD, f"gv_{kind}.npz"))
    rb = 8 if kind == "r8" else 4
    eng = Engine(scenario(gr.NX, gr.NY, 5, gr.NSPEC, [1.0, gr.DY, -20.0, gr.YLAT0]), compute_real_bytes=rb, host_real_bytes=rb,
                 pad=(gr.NXMAX - gr.NX, gr.NYMAX - gr.NY, 0))
    tables, _ = gr.fixture_case(0)
    eng.getvdep_init(tables)
    for t in range(NT):
        _, gin = gr.fixture_case(t)
        frag = fragile(kind, restated(kind, t))
        assert frag.mean() <= (0.0 if kind == "r8" else 0.005)
        for slot in (1, 2):
            got = eng.getvdep(slot, gin, given={k: gin[k] for k in GIVEN})
            w = worst(got["vdep"], gold[f"vdep{t}"])
            bad = w > TOL[kind]
            print(f"device getvdep vs flang fixture {kind} t={t} slot={slot}: max relative deviation {w[~frag].max():.3e} outside reach, "
                  f"{int(frag.sum())} columns within reach of a threshold, {int(bad.sum())} of them beyond the tolerance")
            assert not (bad & ~frag).any(), (t, slot, int((bad & ~frag).sum()), float(w[~frag].max()))
            assert got["device_ms"] > 0
    eng.close()


def chain_inputs(nx=48, ny=32, nz=40):
    ms = [syn.model_levels(nx=nx, ny=ny, nz=nz, phase=p) for p in (0, 4)]
    cins = [syn.calcpar_inputs(m) for m in ms]
    gins = [syn.getvdep_inputs(m, seed=4300 + 10 * s, wftime=10800 * s) for s, m in enumerate(ms)]
    return ms, cins, gins


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_chain_on_the_device(built, kind):
    """verttransform(sfc = NULL) -> calcpar(device_vdep = 1) -> getvdep with nothing but ssr, lsprec, convprec, sd from the
    host: ustar and oli are the ones calcpar left on the device, ps, tt2, td2 the transform's.  Against the restatement
    fed the ustar, oli that calcpar returned."""
    from flexpart_amd.engine import Engine
    nx, ny, nz, nspec = 48, 32, 40, 2
    ms, cins, gins = chain_inputs(nx, ny, nz)
    m, cin, gin = ms[0], cins[0], gins[0]
    rb = 8 if kind == "r8" else 4
    eng = Engine(scenario(nx, ny, nz, nspec, m["geom"], skip=("height", "nmixz")), compute_real_bytes=rb, host_real_bytes=rb)
    tables = syn.getvdep_tables(nx, ny, nspec)
    eng.getvdep_init(tables)
    eng.verttransform(1, m, None, init=True, want=())
    cp = eng.calcpar(1, cin, device_vdep=True)
    got = eng.getvdep(1, gin)
    eng.close()
    full = dict(gin, ustar=cp["ustar"], oli=cp["oli"], ps=m["ps"], tt2=m["tt2"], td2=m["td2"])
    want = gr.getvdep_ref(tables, full, float(m["geom"][1]), float(m["geom"][3]), kind)
    frag = fragile(kind, want)
    assert frag.mean() <= (0.0 if kind == "r8" else 0.005), float(frag.mean())
    w = worst(got["vdep"], want["vdep"])
    print(f"device chain vs restatement {kind}: max relative deviation {w[~frag].max():.3e}, {int(frag.sum())} columns within reach")
    # the gas deposits wherever a column has any land use at all (a few have none), the aerosol settles everywhere
    assert (want["vdep"] >= 0).all() and (want["vdep"][0] > 0).mean() > 0.9 and (want["vdep"][1] > 0).all()
    assert w[~frag].max() <= TOL[kind], float(w[~frag].max())
    assert got["device_ms"] > 0


OUT_PER_CELL = 8


def particle_run(nx=48, ny=32, nz=40):
    """1500 particles, two steps, DRYDEP, two species, and an output grid on which the deposition field is a well-defined
    number: drygridunc is summed with float32 atomic adds (drydepokernel in the step's epilogue), so a cell that takes
    deposits of several particles in one step depends, in its last bits, on the order in which they arrive -- the engine
    run twice on identical input differs from itself there (measured with a random cloud on a 36 x 18 grid: 1 to 5 of 550
    cells, one or two units in the last place).  Here the particles stand on a lattice of 50 x 30 points, 0.9 x 0.65
    met-grid cells apart between 55 S and 55 N, near the ground (four in five inside the deposition layer), and the output
    cells are an eighth of a met-grid cell: a particle moves less than one output cell in two steps, so the 2 x 2 cells
    its deposit is spread over (drydepokernel.f90:41-116) are touched by no other particle.  Every cell then receives at
    most one addend per step and its value does not depend on any order.  pack_runs() checks that this held."""
    sc = syn.small(n=1500, nx=nx, ny=ny, nz=nz, nsteps=2, ctl=5.0, ifine=4, nspec=2)
    sc.update(drydep=1, drydepspec=np.array([1, 1], np.int32))
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    syn.add_outgrid(sc, nxg=OUT_PER_CELL * (nx - 1), nyg=OUT_PER_CELL * (ny - 1), outlon0=xlon0, outlat0=ylat0,
                    dxout=dx / OUT_PER_CELL, dyout=dy / OUT_PER_CELL)
    k = np.arange(1500)
    sc["xtra1"] = 1.5 + 0.9 * (k % 50)
    sc["ytra1"] = 6.0 + 0.65 * (k // 50)
    sc["ztra1"] = np.where(k % 5 == 4, 3000.0, 2.0 + 26.0 * syn._uniform01(1500, 31))
    drop = ("uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep", "height", "nmixz")
    return sc, {k: v for k, v in sc.items() if k not in drop}


@pytest.mark.gpu
def test_guards(built):
    from flexpart_amd.engine import Engine, RNG_TABLE_SEQ
    from flexpart_amd._lib import FpxError
    tables, gin = gr.fixture_case(0)
    given = {k: gin[k] for k in GIVEN}
    geom = [1.0, gr.DY, -20.0, gr.YLAT0]
    # without DRYDEP
    eng = Engine(scenario(gr.NX, gr.NY, 5, gr.NSPEC, geom, drydep=0))
    with pytest.raises(FpxError) as e:
        eng.getvdep(1, gin, given=given)
    assert e.value.code == -1 and "DRYDEP" in str(e.value)
    eng.close()
    # before fpx_getvdep_init; then ustar = NULL without a calcpar of the slot
    eng = Engine(scenario(gr.NX, gr.NY, 5, gr.NSPEC, geom))
    with pytest.raises(FpxError) as e:
        eng.getvdep(1, gin, given=given)
    assert "fpx_getvdep_init" in str(e.value)
    eng.getvdep_init(tables)
    with pytest.raises(FpxError) as e:
        eng.getvdep(1, gin, given={k: gin[k] for k in ("ps", "tt2", "td2")})
    assert e.value.code == -1 and "fpx_calcpar" in str(e.value)
    eng.getvdep(1, gin, given=given)
    eng.close()
    # the stale-slot guard of the step, and calcpar's refusal of a missing vdep
    sc, sce = particle_run()
    ms, cins, gins = chain_inputs()
    eng = Engine(sce, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_TABLE_SEQ)
    eng.getvdep_init(syn.getvdep_tables(48, 32, 2))
    eng.verttransform(1, ms[0], None, init=True, want=())
    with pytest.raises(FpxError) as e:
        eng.calcpar(1, cins[0])                               # DRYDEP, vdep = NULL, device_vdep = 0: as before
    assert e.value.code == -1 and "vdep (the host's getvdep) required" in str(e.value)
    eng.calcpar(1, cins[0], device_vdep=True)
    with pytest.raises(FpxError) as e:
        eng.getvdep(2, gins[1])                               # calcpar ran for slot 1 last, not for slot 2
    assert "fpx_calcpar" in str(e.value)
    eng.getvdep(1, gins[0])
    eng.verttransform(2, ms[1], None, want=())
    eng.calcpar(2, cins[1], device_vdep=True)
    eng.set_windtime(sc["memtime"], sc["memind"])
    eng.upload_particles_from_scenario(sce)
    with pytest.raises(FpxError) as e:
        eng.step(0)                                           # slot 2 still waits for its vdep
    assert "field slots" in str(e.value)
    eng.getvdep(2, gins[1])
    eng.step(0)
    eng.close()


_runs = {}


def pack_runs():
    """1500 particles, two steps, DRYDEP, two species.  Run A: getvdep on the device for both slots, vdep copied back.
    Run B: that copy handed to calcpar(vdep = ..) on the existing path.  Computed once, shared by the two tests below."""
    from flexpart_amd.engine import Engine, RNG_TABLE_SEQ
    if _runs:
        return _runs
    sc, sce = particle_run()
    ms, cins, gins = chain_inputs()
    tables = syn.getvdep_tables(48, 32, 2)
    vd = []
    for run in ("A", "B"):
        eng = Engine(sce, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_TABLE_SEQ)
        if run == "A":
            eng.getvdep_init(tables)
        for s in range(2):
            eng.verttransform(s + 1, ms[s], None, init=(s == 0), want=())
            if run == "A":
                eng.calcpar(s + 1, cins[s], device_vdep=True)
                vd.append(eng.getvdep(s + 1, gins[s])["vdep"])
            else:
                eng.calcpar(s + 1, cins[s], vdep=vd[s])
        eng.set_windtime(sc["memtime"], sc["memind"])
        eng.upload_particles_from_scenario(sce)
        out = eng.run()
        _runs[run] = dict(xmass1=out[-1]["xmass1"], drygridunc=eng.grids()[1])
        eng.close()
        # no two particles within reach of the same output cell, before or after either step (particle_run)
        for x, y in [(sc["xtra1"], sc["ytra1"])] + [(o["xtra1"], o["ytra1"]) for o in out]:
            cx, cy = np.floor(np.asarray(x) * OUT_PER_CELL).astype(np.int64), np.floor(np.asarray(y) * OUT_PER_CELL).astype(np.int64)
            near = (np.abs(cx[:, None] - cx[None, :]) < 3) & (np.abs(cy[:, None] - cy[None, :]) < 3)
            assert near.sum() == near.shape[0], "particles share output cells: drygridunc would depend on the order of the atomics"
    _runs.update(vd=vd, xmass0=np.asarray(sc["xmass1"]).reshape(2, -1))
    return _runs


@pytest.mark.gpu
def test_the_pack_lands_where_the_step_reads_it(built):
    """The masses of all particles after two steps with the device's vdep equal, bit for bit, those of the run that got
    the same vdep through calcpar(vdep = ..): every deposition probability of the step was read from the same numbers."""
    r = pack_runs()
    vd = r["vd"]
    assert not np.array_equal(vd[0], vd[1]) and (vd[0][0] > 0).mean() > 0.9 and (vd[0][1] > 0).all()
    assert (r["A"]["xmass1"] < r["xmass0"]).any() and r["A"]["drygridunc"].sum() > 0       # mass was deposited at all
    assert np.array_equal(r["A"]["xmass1"], r["B"]["xmass1"])


@pytest.mark.gpu
def test_the_deposition_grid_of_the_two_runs_is_bitwise_equal(built):
    """drygridunc of run A and run B, bit for bit (on an output grid where that is well defined: particle_run)."""
    r = pack_runs()
    a, b = r["A"]["drygridunc"], r["B"]["drygridunc"]
    d = np.abs(a - b)
    print(f"drygridunc A vs B: {int((d > 0).sum())} of {int((a != 0).sum())} non-zero cells differ, by at most {float(d.max() / np.abs(a).max()):.3e} of the largest cell")
    assert (a[0, 0, 0, 0] != 0).sum() > 1000 and (a[0, 0, 0, 1] != 0).sum() > 1000       # most particles deposited, both species
    assert np.array_equal(a, b)
