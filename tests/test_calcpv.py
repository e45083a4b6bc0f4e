"""Potential vorticity on model levels on the device (calcpv.f90:42-313, calcpv_nests.f90), run by the two transforms when
fpx_model_levels.pvh is NULL.

Both routines compile with flang in both real kinds, so the row is pinned to the reference itself: the fixtures
tests/golden/pv_r4.npz, pv_r8.npz hold what the unmodified routines return (tests/golden/make_calcpv_golden.py with our
driver ref_pv_driver.f90) for the three cases of synthetic.calcpv_case(), and both the numpy restatement
tests/calcpv_ref.py and the device kernels are compared with them directly.

Errors are relative to the largest |pvh| of the same model level and case (PV grows by orders of magnitude with height).
Tolerances and reach are those of tests/test_getvdep.py: TOL 1e-10 (r8), 2e-4 (r4); REACH 1e-9 (r8), 1e-4 (r4).  The search
for the theta surface is discrete in computed quantities (which bracket holds theta; dt < eps): a point whose margin
(tests/calcpv_ref.py) is below REACH is fragile and may take another path with another libm's pow.  Fragile points that
actually differ are counted and capped (none in r8, where the cases have no fragile point at all; 0.5 % of a case's
points in r4), never masked out silently.

Observed on the CPU, restatement against fixture: r8 worst 2.3e-14, no fragile point; r4 worst
2.1e-5 outside reach, 1922 / 2971 / 1922 fragile points (limited / global / nest) of 21460, one of them beyond TOL in
each case."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import calcpv_ref as pr
from flexpart_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"r8": 1e-10, "r4": 2e-4}
REACH = {"r8": 1e-9, "r4": 1e-4}
CAP = {"r8": 0.0, "r4": 0.005}
KINDS = ["r8", "r4"]
NX, NY, NZ = syn.PV_NX, syn.PV_NY, syn.PV_NZ
EX = pr.CODES["exhausted"]

_cache = {}


def case(name):
    if ("case", name) not in _cache:
        _cache[("case", name)] = syn.calcpv_case(name)
    return _cache[("case", name)]


def restated(kind, name):
    """The restatement of one case, computed once and shared."""
    if (kind, name) not in _cache:
        _cache[(kind, name)] = pr.calcpv_ref(case(name), kind)
    return _cache[(kind, name)]


def golden(kind):
    if ("gold", kind) not in _cache:
        _cache[("gold", kind)] = np.load(os.path.join(GOLD, f"pv_{kind}.npz"))
    return _cache[("gold", kind)]


def maker():
    spec = importlib.util.spec_from_file_location("make_calcpv_golden", os.path.join(GOLD, "make_calcpv_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def judge(kind, name, got, gold, what):
    """Rule 1: every point within TOL of `gold`, except fragile points that actually differ; those are counted and capped."""
    r = restated(kind, name)
    frag = r["margin"] < REACH[kind]
    e = pr.level_error(got, gold)
    bad = e > TOL[kind]
    excused = bad & frag
    print(f"{what} {kind} {name}: worst {e[~frag].max():.3e} outside reach ({e.max():.3e} overall), {int(frag.sum())} fragile points "
          f"of {frag.size}, {int(excused.sum())} of them beyond the tolerance")
    assert np.isfinite(np.asarray(got)).all()
    assert not (bad & ~frag).any(), (name, int((bad & ~frag).sum()), float(e[~frag].max()))
    if kind == "r8":
        assert not frag.any(), (name, int(frag.sum()))               # a condition on the inputs: the case has no fragile point
    assert excused.sum() <= CAP[kind] * frag.size, (name, int(excused.sum()))
    return e


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_reference_fixtures(kind):
    """tests/calcpv_ref.py against the flang build of the unmodified calcpv / calcpv_nests, every point of the three cases."""
    gold = golden(kind)
    base = case("limited")
    for k in ("akz", "bkz", "ps", "tth", "uuh", "vvh"):              # the fixture's inputs are the ones regenerated here, bit for bit
        assert np.array_equal(gold[k], base[k]), k
        assert np.array_equal(case("nest")[k], base[k]), k
        if np.ndim(base[k]) > 1:                                     # 'global': the same with the duplicated meridian
            g = case("global")[k]
            assert np.array_equal(g[..., :-1], base[k][..., :-1]) and np.array_equal(g[..., -1], g[..., 0]), k
    for name in syn.PV_CASES:
        assert np.array_equal(gold[f"geom_{name}"], case(name)["geom"])
        judge(kind, name, restated(kind, name)["pvh"], gold[f"pvh_{name}"].astype(np.float64), "calcpv restatement vs flang fixture")
        assert np.array_equal(gold[f"code_{name}"], restated(kind, name)["code"]), name


@pytest.mark.ref
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_live_reference(kind):
    """The same against the reference compiled on the spot; the committed fixture is what the reference gives."""
    mk = maker()
    if not mk.available():
        pytest.skip("reference sources and flang not present")
    bd = os.path.join(ROOT, "oracle", "_ref", "pvref")
    os.makedirs(bd, exist_ok=True)
    gold = golden(kind)
    for name in syn.PV_CASES:
        nest = name == "nest"
        exe = mk.build(kind, bd, nest=nest, modules_from=os.path.join(ROOT, "oracle", "_ref", f"obj_{kind}" + ("n" if nest else "")))
        live = mk.run(exe, case(name), bd)
        judge(kind, name, restated(kind, name)["pvh"], live, "calcpv restatement vs live flang build")
        assert np.array_equal(live.astype(gold[f"pvh_{name}"].dtype), gold[f"pvh_{name}"]), name


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_covers_every_branch(kind):
    """Counted from the restatement's record of decisions on each fixture case (the fixture carries the same record)."""
    for name in syn.PV_CASES:
        r = restated(kind, name)
        cd, rows = r["code"], slice(1, NY - 1) if name == "global" else slice(0, NY)
        assert np.array_equal(golden(kind)[f"code_{name}"], cd)
        n = {}
        for d, (a, b) in (("x", (0, 1)), ("y", (2, 3))):
            both = np.stack([cd[a], cd[b]])
            n[f"{d}: upward, first test"] = int((both == pr.CODES["up_first"]).sum())
            n[f"{d}: upward, later test"] = int((both == pr.CODES["up_later"]).sum())
            n[f"{d}: downward"] = int((both == pr.CODES["down"]).sum())
            n[f"{d}: exhausted on one side"] = int(((cd[a] == EX) ^ (cd[b] == EX)).sum())
            n[f"{d}: exhausted on both sides"] = int(((cd[a] == EX) & (cd[b] == EX)).sum())
        assert n["x: exhausted on both sides"] == int(r["jux0"].sum()) and n["y: exhausted on both sides"] == int(r["juy0"].sum())
        # kl = 1 (nothing below: every test goes upward) and kl = nuvz (nothing above: every test goes downward)
        n["kl = 1 found upward"] = int(np.isin(cd[:, 0, rows], (1, 2)).sum())
        n["kl = nuvz found downward"] = int((cd[:, NZ - 1, rows] == pr.CODES["down"]).sum())
        assert not (cd[:, 0, rows] == pr.CODES["down"]).any() and not np.isin(cd[:, NZ - 1, rows], (1, 2)).any()
        assert (cd[:, :, rows] != 0).all()                           # every point of every row that is not a pole row was searched
        if name == "global":
            assert (cd[:, :, 0] == 0).all() and (cd[:, :, NY - 1] == 0).all()
            gold = golden(kind)["pvh_global"]
            n["pole rows"] = 2 * int((gold[:, [0, NY - 1], :] == gold[:, [0, NY - 1], :1]).all())
            # the cyclic wrap on both sides: column 0 looks at nx-2, column nx-1 at 1; with the duplicated meridian the
            # two columns are the same point of the globe and get the same PV, bit for bit, in the reference's output
            n["wrap: columns 0 and nx-1 agree"] = int(np.array_equal(gold[:, 1:-1, 0], gold[:, 1:-1, NX - 1])) * (NZ * (NY - 2))
            n["wrap, west: found next door"] = int(np.isin(cd[0][:, rows, 0], (1, 2, 3)).sum())
            n["wrap, east: found next door"] = int(np.isin(cd[1][:, rows, NX - 1], (1, 2, 3)).sum())
        else:
            # edge columns and rows: the virtual neighbour is the column itself, met at the first test (below the top level)
            n["edge columns"] = int((cd[0][: NZ - 1, :, 0] == 1).sum() + (cd[1][: NZ - 1, :, NX - 1] == 1).sum())
            n["edge rows"] = int((cd[2][: NZ - 1, 0, :] == 1).sum() + (cd[3][: NZ - 1, NY - 1, :] == 1).sum())
            assert n["edge columns"] == 2 * (NZ - 1) * NY and n["edge rows"] == 2 * (NZ - 1) * NX
        ties = int(r["tie"].sum())
        print(f"calcpv fixture {kind} {name}: {n}; points with dt < eps: {ties}")
        assert all(v > 0 for v in n.values()), n
        if kind == "r8":                                             # in r4 theta's ulp exceeds eps: only exact ties reach the branch
            for ix, jy, kl in syn.PV_TIES:
                assert r["tie"][kl - 1, jy, ix] and cd[1][kl - 1, jy, ix] == pr.CODES["up_first"], (ix, jy, kl)


def test_new_struct_has_the_size_the_c_compiler_gives_it(tmp_path):
    import subprocess
    from flexpart_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include "flexpart_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(fpx_calcpv_cfg), offsetof(fpx_calcpv_cfg, dxn), sizeof(fpx_model_levels));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off, ml = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_lib.FpxCalcpvCfg) == 8 + 8 * _lib.FPX_MAXNESTS
    assert off == _lib.FpxCalcpvCfg.dxn.offset == 8
    assert ml == C.sizeof(_lib.FpxModelLevels) == 13 * 8 + 4 * 4 + 2 * 8      # unchanged: a NULL pvh needs no new member


def test_abi_version_is_unchanged_and_the_symbols_are_exported(built):
    from flexpart_amd import _lib
    lib = _lib.load()
    assert lib.fpx_abi_version() == 4
    for s in ("fpx_calcpv_init", "fpx_get_pvh", "fpx_calcpv_time"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None


# ---- GPU ---------------------------------------------------------------------------------------------------------
PAD = (syn.PV_NXMAX - NX, syn.PV_NYMAX - NY)
SENTINEL = 7.0


def engine_for(c, kind, sc=None, **kw):
    """An engine on the grid of model-level input c; without sc a run without particles and without fields."""
    from flexpart_amd.engine import Engine, RNG_PHILOX
    nx, ny, nz = (int(v) for v in c["grid"])
    drop = ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "uupol", "vvpol", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep")
    if sc is None:
        sc = syn.small(n=0, nx=nx, ny=ny, nz=nz, nsteps=1)
    sc = {k: v for k, v in dict(sc, grid=c["grid"], geom=c["geom"], globalflags=c["globalflags"]).items() if k not in drop}
    rb = 8 if kind == "r8" else 4
    return Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=RNG_PHILOX, **kw)


def sfc_for(nx, ny, m=0):
    return {k: np.full((ny, nx), v) for k, v in (("hmix", 800.0 + 50.0 * m), ("ustar", 0.3), ("wstar", 1.0), ("oli", 0.01), ("tropopause", 11000.0))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["limited", "global"])
@pytest.mark.parametrize("kind", KINDS)
def test_device_matches_the_reference_fixture(built, kind, name):
    """verttransform(device_pv = True) + get_pvh against what flang's build of the unmodified calcpv returned; arrays of
    40 x 32 for 37 x 29 columns.  The first call hands over a pvh whose padding holds a sentinel: the device's own PV of the
    second call must leave it alone."""
    c = case(name)
    gold = golden(kind)[f"pvh_{name}"].astype(np.float64)
    eng = engine_for(c, kind, pad=PAD + (0,))
    rt = eng.hreal
    host = {"pvh": np.full((NZ, syn.PV_NYMAX, syn.PV_NXMAX), SENTINEL, rt)}
    given = eng.verttransform(1, c, sfc_for(NX, NY), init=True, want=("pv",), host_arrays=host)
    assert given["calcpv_ms"] == 0.0
    assert np.array_equal(eng.get_pvh(), np.asarray(c["pvh"]).astype(rt).astype(np.float64))      # the host's own array comes back
    out = eng.verttransform(1, c, sfc_for(NX, NY), want=("pv",), device_pv=True)
    full = eng.get_pvh(padded=True)
    got = eng.get_pvh()
    eng.close()
    assert out["calcpv_ms"] > 0 and out["device_ms"] > 0
    judge(kind, name, got, gold, "device calcpv vs flang fixture")
    assert (full[:, NY:, :] == SENTINEL).all() and (full[:, :, NX:] == SENTINEL).all()           # padding is not written
    assert not np.array_equal(out["pv"], given["pv"])                                            # the z-level pv follows
    if name == "global":
        scale = np.abs(gold).reshape(NZ, -1).max(axis=1)
        for pole, ring in ((0, 1), (NY - 1, NY - 2)):
            assert (got[:, pole, :] == got[:, pole, :1]).all()                                   # constant along ix
            mean = got[:, ring, :].mean(axis=1)                                                  # of the device's own ring row
            assert (np.abs(got[:, pole, 0] - mean) <= TOL[kind] * scale).all(), float((np.abs(got[:, pole, 0] - mean) / scale).max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_device_nest_matches_the_reference_fixture(built, kind):
    """The nest of the fixture inside the 'limited' grid, through nest= and calcpv_init, against flang's calcpv_nests;
    before fpx_calcpv_init the call is refused with FPX_ERR_STATE."""
    from flexpart_amd._lib import FpxError
    c, n = case("limited"), case("nest")
    gold = golden(kind)["pvh_nest"].astype(np.float64)
    eng = engine_for(c, kind, nest_pad=PAD)
    eng.verttransform(1, c, sfc_for(NX, NY), init=True, want=(), device_pv=True)
    eng.init_nest(n["grid"][:2], n["geom"])
    with pytest.raises(FpxError) as e:
        eng.get_pvh(nest=1)                                          # no transform of the nest yet
    assert e.value.code == -3
    with pytest.raises(FpxError) as e:
        eng.verttransform(1, n, sfc_for(NX, NY), nest=1, want=(), device_pv=True)
    assert e.value.code == -3 and "fpx_calcpv_init" in str(e.value)
    eng.calcpv_init([n["geom"][0]])
    out = eng.verttransform(1, n, sfc_for(NX, NY), nest=1, want=("pv",), device_pv=True)
    full = eng.get_pvh(nest=1, padded=True)
    got = eng.get_pvh(nest=1)
    mother = eng.get_pvh()
    eng.close()
    judge(kind, "nest", got, gold, "device calcpv_nests vs flang fixture")
    judge(kind, "limited", mother, golden(kind)["pvh_limited"].astype(np.float64), "device calcpv (the nest's mother) vs flang fixture")
    assert (full[:, NY:, :] == 0.0).all() and (full[:, :, NX:] == 0.0).all()                     # padding is not written
    assert np.isfinite(out["pv"]).all() and np.abs(out["pv"]).max() > 0


def _chain():
    """Run A: both slots with the PV computed on the device.  Run B: a fresh engine handed what A's get_pvh returned.
    Run C: handed an arbitrary pvh.  300 particles of tests/test_partoutput.py's scenario; computed once and shared."""
    if "chain" in _cache:
        return _cache["chain"]
    import tempfile
    import test_partoutput as tp
    from flexpart_amd._lib import FpxDiagFields
    from flexpart_amd.engine import _vp
    sc = tp.scenario(1, n=300)
    nx, ny, nz = (int(v) for v in sc["grid"])
    ms = [syn.model_levels(nx, ny, nz, phase=p) for p in (0, 4)]
    assert np.array_equal(ms[0]["geom"], sc["geom"]) and np.array_equal(ms[0]["globalflags"], sc["globalflags"])
    want = ("uu", "vv", "ww", "tt", "qv", "pv", "rho", "drhodz")
    res, pvh = {}, []
    with tempfile.TemporaryDirectory() as td:
        for run in ("A", "B", "C"):
            eng = engine_for(ms[0], "r8", sc=sc)
            oro = np.ascontiguousarray(sc["oro"], np.float64)
            f = FpxDiagFields()
            f.oro = _vp(oro)
            assert eng.lib.fpx_upload_diag_fields(eng.h, 0, C.byref(f)) == 0
            outs = []
            for s in (0, 1):
                sfc = {k: sc[k][s] for k in ("hmix", "ustar", "wstar", "oli", "tropopause")}
                m = ms[s] if run != "B" else dict(ms[s], pvh=pvh[s])
                outs.append(eng.verttransform(s + 1, m, sfc, init=(s == 0), want=want, device_pv=(run == "A")))
                if run == "A":
                    pvh.append(eng.get_pvh())
            eng.set_windtime(sc["memtime"], sc["memind"])
            path = os.path.join(td, f"partposit_{run}")
            nrec = eng.partoutput(sc["itime"], path)
            eng.close()
            res[run] = dict(outs=outs, nrec=nrec, file=open(path, "rb").read())
    res["pvh"], res["nparticles"] = pvh, int((sc["itra1"] == sc["itime"]).sum())
    _cache["chain"] = res
    return res


@pytest.mark.gpu
def test_chain_zlevel_pv_and_the_other_outputs(built):
    """The z-level pv of the run that computed pvh on the device equals, bit for bit, that of a fresh engine handed the
    same pvh; every other output of the transform equals that of a run handed an arbitrary pvh."""
    r = _chain()
    for s in (0, 1):
        a, b, c = (r[k]["outs"][s] for k in "ABC")
        assert a["calcpv_ms"] > 0 and b["calcpv_ms"] == 0 and c["calcpv_ms"] == 0
        assert np.array_equal(a["pv"], b["pv"]) and np.abs(a["pv"]).max() > 0
        assert not np.array_equal(a["pv"], c["pv"])
        for k in ("uu", "vv", "ww", "tt", "qv", "rho", "drhodz", "height"):
            assert np.array_equal(a[k], c[k]) and np.array_equal(a[k], b[k]), k
        assert a["nmixz"] == c["nmixz"]
    assert not np.array_equal(r["pvh"][0], r["pvh"][1])


@pytest.mark.gpu
def test_chain_partoutput_files_are_byte_identical(built):
    """fpx_partoutput interpolates the z-level pv the transform left on the device: the dumps of run A and run B are the
    same bytes, and differ from the dump of the run with another pvh."""
    r = _chain()
    assert r["A"]["nrec"] == r["B"]["nrec"] == r["nparticles"] > 100
    assert r["A"]["file"] == r["B"]["file"]
    assert r["A"]["file"] != r["C"]["file"] and len(r["A"]["file"]) == len(r["C"]["file"])


@pytest.mark.gpu
def test_guards(built):
    from flexpart_amd._lib import FpxError
    c = case("limited")
    eng = engine_for(c, "r8")
    with pytest.raises(FpxError) as e:
        eng.get_pvh()                                                # before any transform
    assert e.value.code == -3
    ms = C.c_double(-1.0)
    assert eng.lib.fpx_calcpv_time(eng.h, C.byref(ms)) == 0 and ms.value == 0.0
    out = eng.verttransform(1, c, sfc_for(NX, NY), init=True, want=(), device_pv=True)
    assert out["calcpv_ms"] > 0
    out = eng.verttransform(2, c, sfc_for(NX, NY), want=())           # handed pvh: the time of the PV kernels is 0 again
    assert out["calcpv_ms"] == 0.0
    with pytest.raises(FpxError) as e:
        eng.get_pvh(nest=1)                                          # no such nest
    assert e.value.code == -1
    eng.close()
