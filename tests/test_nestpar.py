"""calcpar_nests and getvdep_nests on the device: fpx_verttransform_nest(sfc = NULL), fpx_calcpar_nest,
fpx_getvdep_nest_init, fpx_getvdep_nest.

getvdep_nests.f90 and all it calls compile with flang in both real kinds: that half is pinned to the reference itself
(tests/golden/gvn_r4.npz, gvn_r8.npz; tests/golden/make_getvdep_nests_golden.py with our driver ref_gvn_driver.f90), and
tests/nestpar_ref.py restates it on top of tests/getvdep_ref.py.  The reference computes the seasonal category of a nest's
row from the MOTHER grid's dy, ylat0 (getvdep_nests.f90:54); the fixture geometry makes that visible (rows 13..23 of the
nest), and the restatement with the nest's own latitude must fail there.

calcpar_nests.f90 calls obukhov.f90 and richardson.f90, which `use class_gribfile` (ecCodes): like calcpar it cannot be
compiled here and is PARITY UNPINNED; its yardstick is oracle/calcpar_oracle.c (cp_oracle) fed the nest's arrays and geometry.

Tolerances and reaches are those of tests/test_getvdep.py and tests/test_calcpar.py: TOL 1e-10 (r8) / 2e-4 (r4), REACH 1e-9 /
1e-4; columns within reach of a discrete decision are counted and capped (getvdep 0 / 0.5 %, calcpar 0 / 25 % with at most
1 % beyond the tolerance), never masked silently.

Shapes: mother grid 24 x 16, nest 1 of 37 x 29 columns in arrays of 48 x 36 (the last block of 256 lanes is partial, the
strides differ from the extents), nest 2 of 21 x 13, 40 levels, four species.  The host's arrays of all nests share one
nxmaxn, nymaxn (fpx_nests, as in par_mod), so nest 2 is held in 48 x 36 as well."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import getvdep_ref as gr
import nestpar_ref as nr
from flexpart_amd import synthetic as syn
from oracle.oracle import cp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"r8": 1e-10, "r4": 2e-4}
REACH = {"r8": 1e-9, "r4": 1e-4}
GV_CAP = {"r8": 0.0, "r4": 0.005}
CP_CAP = {"r8": 0.0, "r4": 0.25}
NT = len(syn.GV_WFTIMES)
GIVEN = ("ustar", "oli", "ps", "tt2", "td2")
CPF = ("ustar", "wstar", "oli", "hmix", "tropopause")
NEST_PAD = (nr.NXMAXN - nr.NXN, nr.NYMAXN - nr.NYN)

_cache = {}


def restated(kind, t, own=False):
    if (kind, t, own) not in _cache:
        tables, gin = nr.fixture_case(t)
        _cache[(kind, t, own)] = nr.getvdep_nests_ref(tables, gin, kind, own_latitude=own)
    return _cache[(kind, t, own)]


def cp_want(which, kind, phase=3):
    """cp_oracle on the nest's arrays and the nest's geom, computed once."""
    key = ("cp", which, kind, phase)
    if key not in _cache:
        n = nr.nest_levels(which, phase)
        _cache[key] = (n, syn.nest_calcpar_inputs(n), cp_oracle(n, syn.nest_calcpar_inputs(n), kind))
    return _cache[key]


def gv_fragile(kind, r):
    return (r["margin_rh"] < REACH[kind]) | (r["margin_alpha"] < REACH[kind])


def worst(got, gold):
    scale = np.abs(gold).reshape(gold.shape[0], -1).max(axis=1)
    scale = np.where(scale > 0, scale, 1.0)[:, None, None]
    return (np.abs(got - gold) / scale).max(axis=0)


def maker():
    spec = importlib.util.spec_from_file_location("make_getvdep_nests_golden", os.path.join(GOLD, "make_getvdep_nests_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_calcpar(got, want, kind, what):
    """The margin rule of tests/test_calcpar.py; returns the worst relative deviation outside reach."""
    fragile = want["margin"] < REACH[kind]
    assert fragile.mean() <= CP_CAP[kind], (what, float(fragile.mean()))
    seen = 0.0
    for k in CPF:
        scale = np.abs(want[k]).max()
        dev = np.abs(got[k] - want[k]) / scale
        bad = dev > TOL[kind]
        seen = max(seen, float(dev[~fragile].max()))
        assert not (bad & ~fragile).any(), (what, k, int((bad & ~fragile).sum()), float(dev[~fragile].max()))
        assert bad.sum() <= (0 if k == "ustar" else 0.01 * want["hmix"].size), (what, k, int(bad.sum()))
    print(f"device calcpar_nest vs restatement {kind} {what}: max relative deviation outside reach {seen:.3e}, {int(fragile.sum())} columns within reach")
    return seen


# ---- CPU ---------------------------------------------------------------------------------------------------------
def test_geometry_makes_the_mother_grid_latitude_visible():
    """At every fixture time at least a third of the nest's rows get another seasonal category from the reference's formula
    (the mother grid's dy, ylat0) than from the nest's own latitude; the nest lies inside the mother grid."""
    dx, dy, xlon0, ylat0 = nr.GEOM
    for (nxn, nyn), (dxn, dyn, x0n, y0n) in (((nr.NXN, nr.NYN), nr.NESTGEOM), ((nr.NXN2, nr.NYN2), nr.NESTGEOM2)):
        assert x0n >= xlon0 and x0n + (nxn - 1) * dxn <= xlon0 + (nr.NX - 1) * dx
        assert y0n >= ylat0 and y0n + (nyn - 1) * dyn <= ylat0 + (nr.NY - 1) * dy
    for t in range(NT):
        for kind in ("r8", "r4"):
            a, b = nr.season_rows(syn.GV_WFTIMES[t], kind)
            print(f"t={t} {kind}: rows whose season differs: {np.flatnonzero(a != b).tolist()}")
            assert (a != b).mean() >= 1.0 / 3.0, (t, kind, float((a != b).mean()))


@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_restatement_matches_reference_fixtures(kind):
    """tests/nestpar_ref.py against the flang build of the unmodified getvdep_nests, every species and column of the three
    wind-field times; with the nest's own latitude it fails on the rows whose season differs, and only there."""
    gold = np.load(os.path.join(GOLD, f"gvn_{kind}.npz"))
    seen = 0.0
    for t in range(NT):
        tables, gin = nr.fixture_case(t)
        for k in nr.FIELDS:
            assert np.array_equal(gold[f"{k}{t}"], gin[k]), k
        assert int(gold[f"wftime{t}"]) == gin["wftime"]
        for k in nr.TABLES:
            assert np.array_equal(gold[k], tables[k]), k
        r = restated(kind, t)
        w = worst(r["vdep"], gold[f"vdep{t}"])
        seen = max(seen, float(w.max()))
        assert w.max() <= TOL[kind], (t, float(w.max()))
        a, b = nr.season_rows(syn.GV_WFTIMES[t], kind)
        wo = worst(restated(kind, t, own=True)["vdep"], gold[f"vdep{t}"])
        assert wo[a == b].max() <= TOL[kind]
        rows_off = (wo > TOL[kind]).any(axis=1)
        print(f"getvdep_nests restatement vs flang fixture {kind} t={t}: max relative deviation {w.max():.3e}; with the nest's own latitude "
              f"{wo.max():.3e}, rows off {np.flatnonzero(rows_off).tolist()}")
        assert rows_off[a != b].all() and wo.max() > 100 * TOL[kind], (t, np.flatnonzero(rows_off).tolist())
    print(f"getvdep_nests restatement vs flang fixture {kind}: max over all times {seen:.3e}")


@pytest.mark.ref
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_restatement_matches_live_reference(kind):
    """The same against the reference compiled on the spot, for another draw of the inputs."""
    mk = maker()
    if not mk.available():
        pytest.skip("reference sources and flang not present")
    bd = os.path.join(ROOT, "oracle", "_ref", "gvnref")
    os.makedirs(bd, exist_ok=True)
    exe = mk.build(kind, bd, modules_from=os.path.join(ROOT, "oracle", "_ref", f"obj_{kind}n"))
    geo = (nr.GEOM[1], nr.GEOM[3], nr.NESTGEOM[1], nr.NESTGEOM[3])
    tables = syn.getvdep_tables(nr.NXN, nr.NYN, nr.NSPEC, seed=4150)
    gin = syn.nest_getvdep_inputs((nr.NYN, nr.NXN), seed=977, wftime=syn.GV_WFTIMES[1])
    live = mk.run(exe, tables, gin, *geo, bd)
    r = nr.getvdep_nests_ref(tables, gin, kind)
    ok = ~gv_fragile(kind, r)
    w = worst(r["vdep"], live)
    assert w[ok].max() <= TOL[kind], float(w[ok].max())
    assert (~ok).mean() <= GV_CAP[kind]
    t, g0 = nr.fixture_case(0)
    gold = np.load(os.path.join(GOLD, f"gvn_{kind}.npz"))
    assert np.array_equal(mk.run(exe, t, g0, *geo, bd), gold["vdep0"])     # the committed fixture is what the reference gives


def test_fixture_inputs_stay_inside_the_caps():
    """By the restatements' own margins: the share of columns within reach of a discrete decision, for the getvdep_nests
    fixture and for the model levels the calcpar_nest tests use (both nests, both real kinds)."""
    for t in range(NT):
        for kind in ("r8", "r4"):
            frac = float(gv_fragile(kind, restated(kind, t)).mean())
            print(f"getvdep_nests fixture t={t} {kind}: share of columns within {REACH[kind]:g} of a threshold {frac:.5f}")
            assert frac <= GV_CAP[kind], (t, kind, frac)
    for which in (1, 2):
        for kind in ("r8", "r4"):
            _, _, want = cp_want(which, kind)
            frac = float((want["margin"] < REACH[kind]).mean())
            print(f"calcpar nest {which} {kind}: share of columns within {REACH[kind]:g} of a level-search threshold {frac:.5f}")
            assert frac <= CP_CAP[kind], (which, kind, frac)
            assert (want["tropopause"] > 0).all()                # every column of the ordinary fields has a tropopause


def stale_case():
    """Second wind field of the stale-tropopause test: a block and a few single columns of nest 1 without any layer that
    meets the criterion."""
    mask = np.zeros((nr.NYN, nr.NXN), bool)
    mask[10:14, 5:9] = True
    mask[0, 0] = mask[nr.NYN - 1, nr.NXN - 1] = mask[20, 30] = True
    n2 = syn.no_tropopause_columns(nr.nest_levels(1, phase=7), mask)
    return mask, n2, syn.nest_calcpar_inputs(n2)


def test_columns_without_a_tropopause_exist():
    """cp_oracle leaves the tropopause of exactly the prepared columns untouched (zero, as it starts)."""
    mask, n2, c2 = stale_case()
    want = cp_oracle(n2, c2, "r8")
    assert np.array_equal(want["tropopause"] == 0.0, mask) and mask.sum() == 19
    assert (want["margin"] < REACH["r8"]).sum() == 0


def test_structs_and_abi_are_unchanged(built, tmp_path):
    import subprocess
    from flexpart_amd import _lib
    pairs = [("fpx_getvdep_tables", _lib.FpxGetvdepTables), ("fpx_getvdep_in", _lib.FpxGetvdepIn), ("fpx_calcpar_in", _lib.FpxCalcparIn),
             ("fpx_calcpar_out", _lib.FpxCalcparOut), ("fpx_model_levels", _lib.FpxModelLevels), ("fpx_fields", _lib.FpxFields), ("fpx_config", _lib.FpxConfig)]
    src = tmp_path / "sizes.c"
    src.write_text('#include "flexpart_amd.h"\n#include <stdio.h>\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n, _ in pairs)
                   + "  int (*a)(fpx_handle, int32_t, int32_t, const fpx_calcpar_in *, const fpx_calcpar_out *) = fpx_calcpar_nest;\n"
                   + "  int (*b)(fpx_handle, int32_t, const void *) = fpx_getvdep_nest_init;\n"
                   + "  int (*c)(fpx_handle, int32_t, int32_t, const fpx_getvdep_in *, void *) = fpx_getvdep_nest;\n"
                   + "  return !(a && b && c);\n}\n")
    # the prototypes of the three new entry points are what the header declares (the initialisers above), and the sizes
    # the C compiler gives the structs are the ones they had before: a static assertion each
    sizes = {"fpx_getvdep_tables": 4 * 4 + 8 + 16 * 8, "fpx_getvdep_in": 8 + 9 * 8, "fpx_calcpar_in": 6 * 8 + 4 * 4, "fpx_calcpar_out": 5 * 8,
             "fpx_model_levels": 13 * 8 + 4 * 4 + 2 * 8, "fpx_fields": 14 * 8, "fpx_config": C.sizeof(_lib.FpxConfig)}
    with open(src, "a") as f:
        for n, _ in pairs:
            f.write(f"typedef char size_of_{n}[sizeof({n}) == {sizes[n]} ? 1 : -1];\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-Wno-unused-local-typedefs", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes.o")])
    for n, t in pairs:
        assert sizes[n] == C.sizeof(t), n
    lib = _lib.load()
    assert lib.fpx_abi_version() == 4
    for name in ("fpx_calcpar_nest", "fpx_getvdep_nest_init", "fpx_getvdep_nest", "fpx_verttransform_nest"):
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    assert "stay the host's" not in hdr and "fpx_getvdep_nest" in hdr


# ---- GPU ---------------------------------------------------------------------------------------------------------
def scenario(nx, ny, nz, nspec, geom, drydep=1, **extra):
    """A run without particles and without fields: grid, switches and the species of a DRYDEP run."""
    sc = dict(grid=np.array([nx, ny, nz], np.int32), geom=np.asarray(geom, np.float64), globalflags=np.zeros(3, np.int32), nspec=nspec, npart=0)
    skip = ("uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep", "height", "nmixz")
    sc.update({k: v for k, v in syn.base_scenario(8, 6, nz, nspec=nspec).items() if k not in sc and k not in skip})
    sc.update(drydep=drydep, drydepspec=np.full(nspec, drydep, np.int32))
    sc.update(extra)
    return sc


def mother_tables(ntab):
    """The tables fpx_getvdep_init gets: the small ones of the nest case (com_mod has one set for all grids) with a land-use
    inventory of the mother grid's own."""
    return dict(ntab, xlanduse=syn.getvdep_tables(nr.NX, nr.NY, nr.NSPEC)["xlanduse"])


def nest_engine(kind, nests=1, drydep=1, sc=None, **kw):
    """An engine on the fixture's mother grid with nest 1 (and nest 2), the mother grid transformed once (the z levels)."""
    from flexpart_amd.engine import Engine
    rb = 8 if kind == "r8" else 4
    eng = Engine(sc or scenario(nr.NX, nr.NY, nr.NZ, nr.NSPEC, nr.GEOM, drydep=drydep), compute_real_bytes=rb, host_real_bytes=rb, nest_pad=NEST_PAD, **kw)
    eng.init_nests([((nr.NXN, nr.NYN), nr.NESTGEOM), ((nr.NXN2, nr.NYN2), nr.NESTGEOM2)][:nests])
    eng.verttransform(1, nr.mother_levels(), None, init=True, want=())
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_calcpar_nest_matches_the_restatement(built, kind):
    """fpx_verttransform_nest(sfc = NULL) + fpx_calcpar_nest against cp_oracle on the nest's arrays and geometry, into slot 1
    and slot 2.  Observed worst deviation outside reach: see DESIGN section 25."""
    n, cin, want = cp_want(1, kind)
    eng = nest_engine(kind, drydep=0)
    for slot in (1, 2):
        eng.verttransform(slot, n, None, nest=1, want=())
        got = eng.calcpar_nest(1, slot, cin)
        check_calcpar(got, want, kind, f"slot {slot}")
        assert got["device_ms"] > 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_same_numbers_same_bits(built, kind):
    """The nest calls of engine A and the mother-grid calls of an engine whose mother grid has the nest's extent, strides and
    numbers give the same bits: the five calcpar fields (B1: the nest's geometry, which sets altmin) and vdep (B2: the dy,
    ylat0 of A's mother grid, which set the season)."""
    from flexpart_amd.engine import Engine
    rb = 8 if kind == "r8" else 4
    n, cin, _ = cp_want(1, kind)
    tables = syn.getvdep_tables(nr.NXN, nr.NYN, nr.NSPEC, seed=4150)
    gin = syn.nest_getvdep_inputs(n, seed=4350, wftime=syn.GV_WFTIMES[1])
    a = nest_engine(kind)
    a.getvdep_init(mother_tables(tables))
    a.getvdep_nest_init(1, tables["xlanduse"])
    a.verttransform(1, n, None, nest=1, want=())
    cpa = a.calcpar_nest(1, 1, cin, device_vdep=True)
    vda = a.getvdep_nest(1, 1, gin)["vdep"]
    a.close()
    pad = (NEST_PAD[0], NEST_PAD[1], 0)
    b1 = Engine(scenario(nr.NXN, nr.NYN, nr.NZ, nr.NSPEC, nr.NESTGEOM, drydep=0), compute_real_bytes=rb, host_real_bytes=rb, pad=pad)
    b1.verttransform(1, n, None, init=True, want=())
    cpb = b1.calcpar(1, cin)
    b1.close()
    for k in CPF:
        assert np.array_equal(cpa[k], cpb[k]), k
    b2 = Engine(scenario(nr.NXN, nr.NYN, nr.NZ, nr.NSPEC, [nr.NESTGEOM[0], nr.GEOM[1], nr.NESTGEOM[2], nr.GEOM[3]]), compute_real_bytes=rb, host_real_bytes=rb, pad=pad)
    b2.getvdep_init(tables)
    b2.verttransform(1, n, None, init=True, want=())
    b2.calcpar(1, cin, device_vdep=True)
    vdb = b2.getvdep(1, gin)["vdep"]
    b2.close()
    assert (vda[0] > 0).mean() > 0.9 and np.array_equal(vda, vdb)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_getvdep_nest_matches_the_reference_fixture(built, kind):
    """fpx_getvdep_nest with all of ustarn, olin, psn, tt2n, td2n given, against what flang's build of the unmodified
    getvdep_nests returned: three wind-field times, each into slot 1 and slot 2.  A build that took the season from the nest's
    own latitude fails here on rows 13..23.  Observed worst deviation outside reach: see DESIGN section 25."""
    gold = np.load(os.path.join(GOLD, f"gvn_{kind}.npz"))
    eng = nest_engine(kind)
    tables, _ = nr.fixture_case(0)
    eng.getvdep_init(mother_tables(tables))
    eng.getvdep_nest_init(1, tables["xlanduse"])
    for t in range(NT):
        _, gin = nr.fixture_case(t)
        frag = gv_fragile(kind, restated(kind, t))
        assert frag.mean() <= GV_CAP[kind]
        for slot in (1, 2):
            got = eng.getvdep_nest(1, slot, gin, given={k: gin[k] for k in GIVEN})
            w = worst(got["vdep"], gold[f"vdep{t}"])
            bad = w > TOL[kind]
            print(f"device getvdep_nest vs flang fixture {kind} t={t} slot={slot}: max relative deviation {w[~frag].max():.3e} outside reach, "
                  f"{int(frag.sum())} columns within reach of a threshold, {int(bad.sum())} of them beyond the tolerance")
            assert not (bad & ~frag).any(), (t, slot, int((bad & ~frag).sum()), float(w[~frag].max()))
            assert got["device_ms"] > 0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_chain_on_the_device(built, kind):
    """transform(sfc = NULL) -> calcpar_nest(device_vdep) -> getvdep_nest with nothing given equals the call that is given the
    restatement's ustarn, olin (and the host's psn, tt2n, td2n), within TOL outside reach."""
    n, cin, want = cp_want(1, kind)
    tables = syn.getvdep_tables(nr.NXN, nr.NYN, nr.NSPEC, seed=4150)
    gin = syn.nest_getvdep_inputs(n, seed=4350, wftime=syn.GV_WFTIMES[2])
    eng = nest_engine(kind)
    eng.getvdep_init(mother_tables(tables))
    eng.getvdep_nest_init(1, tables["xlanduse"])
    eng.verttransform(1, n, None, nest=1, want=())
    eng.calcpar_nest(1, 1, cin, device_vdep=True)
    chain = eng.getvdep_nest(1, 1, gin)["vdep"]
    full = dict(gin, ustar=want["ustar"], oli=want["oli"], ps=n["ps"], tt2=n["tt2"], td2=n["td2"])
    given = eng.getvdep_nest(1, 1, gin, given={k: full[k] for k in GIVEN})["vdep"]
    eng.close()
    frag = gv_fragile(kind, nr.getvdep_nests_ref(tables, full, kind)) | (want["margin"] < REACH[kind])
    assert (gv_fragile(kind, nr.getvdep_nests_ref(tables, full, kind))).mean() <= GV_CAP[kind]
    w = worst(chain, given)
    print(f"device chain vs given {kind}: max relative deviation {w[~frag].max():.3e}, {int(frag.sum())} columns within reach")
    assert (given[1] > 0).all() and w[~frag].max() <= TOL[kind], float(w[~frag].max())


def grid_inputs(g):
    """model levels, calcpar inputs, land use and getvdep inputs of grid g (0: the mother grid, 1, 2: the nests)."""
    m = nr.mother_levels() if g == 0 else nr.nest_levels(g)
    nx, ny = int(m["grid"][0]), int(m["grid"][1])
    cin = syn.calcpar_inputs(m) if g == 0 else syn.nest_calcpar_inputs(m)
    return m, cin, syn.getvdep_tables(nx, ny, nr.NSPEC, seed=4100 + 50 * g), syn.getvdep_inputs(m, seed=4400 + 10 * g, wftime=syn.GV_WFTIMES[g])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_two_nests_and_the_mother_grid_interleaved(built, kind):
    """calcpar for nest 2, the mother grid, nest 1, then getvdep in the opposite order (all from the device's own ustar, oli,
    ps, tt2, td2): each grid's fields are bitwise what they are when that grid runs alone."""
    inp = {g: grid_inputs(g) for g in (0, 1, 2)}

    def start():
        eng = nest_engine(kind, nests=2)
        eng.getvdep_init(inp[0][2])
        for g in (1, 2):
            eng.getvdep_nest_init(g, inp[g][2]["xlanduse"])
        return eng

    def transform(eng, g):
        if g:
            eng.verttransform(1, inp[g][0], None, nest=g, want=())

    def calcpar(eng, g):
        return eng.calcpar(1, inp[g][1], device_vdep=True) if g == 0 else eng.calcpar_nest(g, 1, inp[g][1], device_vdep=True)

    def getvdep(eng, g):
        return (eng.getvdep(1, inp[g][3]) if g == 0 else eng.getvdep_nest(g, 1, inp[g][3]))["vdep"]

    alone = {}
    for g in (0, 1, 2):
        eng = start()
        transform(eng, g)
        alone[g] = (calcpar(eng, g), getvdep(eng, g))
        eng.close()
    eng = start()
    for g in (1, 2):
        transform(eng, g)
    cp = {g: calcpar(eng, g) for g in (2, 0, 1)}
    vd = {g: getvdep(eng, g) for g in (1, 0, 2)}
    eng.close()
    for g in (0, 1, 2):
        for k in CPF:
            assert np.array_equal(cp[g][k], alone[g][0][k]), (g, k)
        assert (vd[g][1] > 0).all() and np.array_equal(vd[g], alone[g][1]), g
    assert cp[1]["hmix"].shape == (nr.NYN, nr.NXN) and cp[2]["hmix"].shape == (nr.NYN2, nr.NXN2)


@pytest.mark.gpu
def test_stale_tropopause(built):
    """The second wind field of slot 1 has columns in which no layer meets the criterion: they keep the first field's value,
    all others take the second field's.  (That the slot-1 pack holds the same numbers as out->tropopause is the subject of
    test_end_to_end, whose slot 1 receives these two fields.)"""
    kind = "r8"
    n1, c1, want1 = cp_want(1, kind)
    mask, n2, c2 = stale_case()
    want2 = cp_oracle(n2, c2, kind)
    eng = nest_engine(kind, drydep=0)
    eng.verttransform(1, n1, None, nest=1, want=())
    t1 = eng.calcpar_nest(1, 1, c1)["tropopause"]
    eng.verttransform(1, n2, None, nest=1, want=())
    t2 = eng.calcpar_nest(1, 1, c2)["tropopause"]
    eng.verttransform(2, n2, None, nest=1, want=())
    t2_slot2 = eng.calcpar_nest(1, 2, c2)["tropopause"]
    eng.close()
    assert (t1 > 0).all() and np.abs(t1 - want1["tropopause"]).max() <= TOL[kind] * want1["tropopause"].max()
    assert np.array_equal(t2[mask], t1[mask])
    assert np.abs(t2 - want2["tropopause"])[~mask].max() <= TOL[kind] * want2["tropopause"].max()
    assert np.all(t2_slot2[mask] == 0.0) and np.array_equal(t2_slot2[~mask], t2[~mask])     # slot 2 never saw the first field


OUT_PER_CELL = 16


def particle_run():
    """1500 particles on a lattice inside nest 1, two steps, DRYDEP, four species; every fifth particle between 8 and 14 km
    (around the tropopause), the others in or near the deposition layer.  The output cells are a sixteenth of a mother cell
    and the lattice points 5.4 x 7.0 output cells apart: no two particles deposit into the same cell, so drygridunc (float32
    atomic adds) does not depend on any order (tests/test_getvdep.py, particle_run); e2e_runs() checks that this held."""
    sc = syn.small(n=1500, nx=nr.NX, ny=nr.NY, nz=nr.NZ, nsteps=2, ctl=5.0, ifine=4, nspec=nr.NSPEC, global_grid=False)
    sc["geom"] = np.array(nr.GEOM, np.float64)
    sc.update(drydep=1, drydepspec=np.ones(nr.NSPEC, np.int32))
    dx, dy, xlon0, ylat0 = nr.GEOM
    syn.add_outgrid(sc, nxg=OUT_PER_CELL * (nr.NX - 1), nyg=OUT_PER_CELL * (nr.NY - 1), outlon0=xlon0, outlat0=ylat0,
                    dxout=dx / OUT_PER_CELL, dyout=dy / OUT_PER_CELL)
    k = np.arange(1500)
    sc["xtra1"] = 2.5 + 0.34 * (k % 50)                  # nest 1 covers 2 .. 20 x 1 .. 15 in mother grid units
    sc["ytra1"] = 1.5 + 0.44 * (k // 50)
    sc["ztra1"] = np.where(k % 5 == 4, 8000.0 + 6000.0 * syn._uniform01(1500, 32), 2.0 + 26.0 * syn._uniform01(1500, 31))
    drop = ("uu", "vv", "ww", "rho", "drhodz", "tt", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep", "height", "nmixz")
    return sc, {k: v for k, v in sc.items() if k not in drop}


_runs = {}


def e2e_runs():
    """Run A: the nest's boundary-layer fields and vdepn computed on the device (slot 1 twice: an earlier wind field, then one
    with columns that keep its tropopause).  Run B: the arrays fpx_calcpar_out / vdep_out returned to A, handed to
    fpx_verttransform_nest(sfc = ..).  The mother grid goes the device chain in both."""
    from flexpart_amd.engine import RNG_TABLE_SEQ
    if _runs:
        return _runs
    sc, sce = particle_run()
    ms = [nr.mother_levels(phase=p) for p in (0, 4)]
    mcin = [syn.calcpar_inputs(m) for m in ms]
    mgin = [syn.getvdep_inputs(m, seed=4300 + 10 * s, wftime=10800 * s) for s, m in enumerate(ms)]
    n0 = nr.nest_levels(1, phase=3)
    mask, n1, _ = stale_case()
    ns = [n1, nr.nest_levels(1, phase=11)]
    ncin = [syn.nest_calcpar_inputs(n) for n in ns]
    ngin = [syn.nest_getvdep_inputs(n, seed=4350 + 10 * s, wftime=10800 * s) for s, n in enumerate(ns)]
    mtab = syn.getvdep_tables(nr.NX, nr.NY, nr.NSPEC)
    ntab = syn.getvdep_tables(nr.NXN, nr.NYN, nr.NSPEC, seed=4150)
    sfc = []
    for run in ("A", "B"):
        eng = nest_engine("r8", sc=sce, rng_mode=RNG_TABLE_SEQ)
        eng.getvdep_init(mtab)
        for s in range(2):
            eng.verttransform(s + 1, ms[s], None, init=False, want=())
            eng.calcpar(s + 1, mcin[s], device_vdep=True)
            eng.getvdep(s + 1, mgin[s])
        if run == "A":
            eng.getvdep_nest_init(1, ntab["xlanduse"])
            eng.verttransform(1, n0, None, nest=1, want=())
            first = eng.calcpar_nest(1, 1, syn.nest_calcpar_inputs(n0), device_vdep=True)
            for s in range(2):
                eng.verttransform(s + 1, ns[s], None, nest=1, want=())
                f = eng.calcpar_nest(1, s + 1, ncin[s], device_vdep=True)
                f["vdep"] = eng.getvdep_nest(1, s + 1, ngin[s])["vdep"]
                sfc.append(f)
            _runs["stale_kept"] = bool(np.array_equal(sfc[0]["tropopause"][mask], first["tropopause"][mask]) and (sfc[0]["tropopause"][mask] > 0).all())
        else:
            for s in range(2):
                eng.verttransform(s + 1, ns[s], {k: sfc[s][k] for k in CPF + ("vdep",)}, nest=1, want=())
        eng.set_windtime(sc["memtime"], sc["memind"])
        eng.upload_particles_from_scenario(sce)
        out = eng.run()
        _runs[run] = dict(out=out[-1], drygridunc=eng.grids()[1])
        eng.close()
        for x, y in [(sc["xtra1"], sc["ytra1"])] + [(o["xtra1"], o["ytra1"]) for o in out]:
            cx, cy = np.floor(np.asarray(x) * OUT_PER_CELL).astype(np.int64), np.floor(np.asarray(y) * OUT_PER_CELL).astype(np.int64)
            near = (np.abs(cx[:, None] - cx[None, :]) < 3) & (np.abs(cy[:, None] - cy[None, :]) < 3)
            assert near.sum() == near.shape[0], "particles share output cells: drygridunc would depend on the order of the atomics"
            assert np.asarray(x).min() > 2.0 and np.asarray(x).max() < 20.0 and np.asarray(y).min() > 1.0 and np.asarray(y).max() < 15.0   # inside nest 1
    _runs.update(xmass0=np.asarray(sc["xmass1"]).reshape(nr.NSPEC, -1), sfc=sfc)
    return _runs


@pytest.mark.gpu
def test_end_to_end(built):
    """Particles and drygridunc of run A and run B (e2e_runs) are bitwise equal: the step read the same numbers from the packs
    fpx_calcpar_nest / fpx_getvdep_nest wrote as from the packs the upload path wrote from their copies -- the slot-1
    tropopause with its stale columns included."""
    r = e2e_runs()
    a, b = r["A"], r["B"]
    assert r["stale_kept"]
    assert (a["out"]["xmass1"] < r["xmass0"]).any() and a["drygridunc"].sum() > 0          # mass was deposited at all
    assert not np.array_equal(r["sfc"][0]["vdep"], r["sfc"][1]["vdep"])
    for k in ("xtra1", "ytra1", "ztra1", "xmass1"):
        assert np.array_equal(a["out"][k], b["out"][k]), k
    assert np.array_equal(a["drygridunc"], b["drygridunc"])


@pytest.mark.gpu
def test_guards(built):
    from flexpart_amd.engine import RNG_TABLE_SEQ
    from flexpart_amd._lib import FpxError
    n, cin, _ = cp_want(1, "r8")
    n2, cin2 = nr.nest_levels(2), syn.nest_calcpar_inputs(nr.nest_levels(2))
    ntab = syn.getvdep_tables(nr.NXN, nr.NYN, nr.NSPEC, seed=4150)
    gin = syn.nest_getvdep_inputs(n, seed=4350, wftime=0)
    sfc = {k: np.full((nr.NYN, nr.NXN), v) for k, v in (("hmix", 800.0), ("ustar", 0.3), ("wstar", 1.0), ("oli", 0.01), ("tropopause", 10000.0))}
    sfc["vdep"] = np.full((nr.NSPEC, nr.NYN, nr.NXN), 0.002)

    def refused(code, text, f, *a, **kw):
        with pytest.raises(FpxError) as e:
            f(*a, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    sc, sce = particle_run()
    eng = nest_engine("r8", nests=2, sc=sce, rng_mode=RNG_TABLE_SEQ)
    m = nr.mother_levels()
    mtab = syn.getvdep_tables(nr.NX, nr.NY, nr.NSPEC)
    refused(-3, "fpx_getvdep_init", eng.getvdep_nest_init, 1, ntab["xlanduse"])
    eng.getvdep_init(mtab)
    for s in (1, 2):
        eng.verttransform(s, m, None, want=())
        eng.calcpar(s, syn.calcpar_inputs(m), device_vdep=True)
        eng.getvdep(s, syn.getvdep_inputs(m))
        eng.verttransform(s, n2, {k: v[..., : nr.NYN2, : nr.NXN2] for k, v in sfc.items()}, nest=2, want=())    # the existing path still loads the slot
    refused(-1, "nest out of range", eng.calcpar_nest, 3, 1, cin, device_vdep=True)
    refused(-1, "nest out of range", eng.getvdep_nest, 0, 1, gin)
    refused(-3, "fpx_verttransform_nest of this nest and slot first", eng.calcpar_nest, 1, 1, cin, device_vdep=True)     # never transformed
    eng.verttransform(1, n, sfc, nest=1, want=())
    eng.verttransform(2, n, None, nest=1, want=())
    refused(-3, "fpx_verttransform_nest of this nest and slot first", eng.calcpar_nest, 1, 1, cin, device_vdep=True)     # slot 2 was the last into the nest's buffers
    refused(-1, "are required", eng.calcpar_nest, 1, 2, dict(cin, sshf=None), device_vdep=True)
    refused(-1, "excessoron required", eng.calcpar_nest, 1, 2, dict(cin, excessoro=None), device_vdep=True)
    refused(-1, "vdepn (the host's getvdep_nests) required", eng.calcpar_nest, 1, 2, cin)
    eng.set_windtime(sc["memtime"], sc["memind"])
    eng.upload_particles_from_scenario(sce)
    refused(-3, "nest fields missing", eng.step, 0)                      # slot 2 of nest 1: transformed with sfc = NULL, no calcpar_nest yet
    eng.calcpar_nest(1, 2, cin, device_vdep=True)
    refused(-3, "nest fields missing", eng.step, 0)                      # ... and still waits for its vdepn
    refused(-3, "fpx_getvdep_nest_init of this nest", eng.getvdep_nest, 1, 2, gin)
    eng.getvdep_nest_init(1, ntab["xlanduse"])
    refused(-1, "fpx_calcpar_nest of this nest and slot first", eng.getvdep_nest, 1, 1, gin)   # calcpar_nest ran for slot 2 last
    refused(-1, "are required", eng.getvdep_nest, 1, 2, dict(gin, sd=None))
    eng.getvdep_nest(1, 2, gin)
    eng.step(0)
    eng.close()
    eng = nest_engine("r8", drydep=0)
    refused(-1, "DRYDEP", eng.getvdep_nest, 1, 1, gin)
    eng.close()
