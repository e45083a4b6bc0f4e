"""calcpar for NCEP GFS fields (the GRIBFILE_CENTRE_NCEP branch of calcpar.f90, obukhov.f90, richardson.f90) on the device:
fpx_calcpar_gfs after fpx_verttransform_gfs.

calcpar.f90, obukhov.f90 and richardson.f90 `use class_gribfile`, whose source needs ecCodes; they take nothing from it but
three integer parameters, so with tests/golden/class_gribfile_standin.f90 the unmodified routines compile (flang, both real
kinds) and everything here is pinned to them: tests/golden/cpg_<case>_<kind>.npz holds what calcpar left after each of three
consecutive calls (slot 1, slot 2, slot 1 again -- the tropopause of a slot persists where the criterion does not fire) of
the cases of tests/calcpar_gfs_ref.py, cp_ecmwf_<kind>.npz one call of the ECMWF branch (make_cpg_golden.py, ref_cpg_driver.f90).

CPU (-m "not gpu"): the numpy restatement and the column body of the kernel compiled for the host (calcpar_gfs_host.cpp) both
equal the fixtures bit for bit -- every field, every call, both kinds, all cases; no column needs the margin rule.  The ECMWF
by-product: oracle.cp_oracle equals the unmodified routine bit for bit in ustar, oli, wstar, hmix.
GPU (-m gpu): the device against the restatement under the rule and the numbers of
tests/test_calcpar.py::test_device_calcpar_matches_the_restatement; the gather packs through trajectories; the stale-slot
guard; the refusals."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import calcpar_gfs_ref as cr
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ["r8", "r4"]
RUN_IDS = [f"{c}-ls{ls}" for c, ls in cr.RUNS]
_cache = {}


def restated(case, ls, kind):
    """The three calls of a run in the restatement, computed once and shared: [(fields, rec)] * 3."""
    if (case, ls, kind) not in _cache:
        _cache[(case, ls, kind)] = cr.run_case(case, ls, kind)
    return _cache[(case, ls, kind)]


def golden(name, kind):
    if (name, kind) not in _cache:
        _cache[(name, kind)] = np.load(os.path.join(GOLD, f"{name}_{kind}.npz"))
    return _cache[(name, kind)]


def maker():
    spec = importlib.util.spec_from_file_location("make_cpg_golden", os.path.join(GOLD, "make_cpg_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("run", cr.RUNS, ids=RUN_IDS)
def test_restatement_equals_reference_fixture(run, kind):
    case, ls = run
    g = golden(f"cpg_{case}", kind)
    for n, (f, rec) in enumerate(restated(case, ls, kind)):
        for k in cr.FIELDS:
            assert np.isfinite(f[k]).all(), (n, k)
            want = g[f"{k}_{n}_ls{ls}"].astype(np.float64)
            assert np.array_equal(f[k], want), (n, k, int((f[k] != want).sum()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("run", cr.RUNS, ids=RUN_IDS)
def test_inputs_meet_the_conditions(run, kind):
    """The conditions on the synthetic inputs, again from the restatement's record (the fixture script asserts them before it
    writes): kzmin found in every column, the two llev differ somewhere, llev takes four values in `terrain`, both hmix clamps,
    both signs and zero of sshf, the three altmin branches, both outcomes of |tv - tvold| > 0.2, the shares of fragile
    columns the GPU test allows.  The third call shows the persistence: a column whose criterion does not fire holds the
    tropopause the first call left in slot 1, not zero."""
    case, ls = run
    outs = restated(case, ls, kind)
    unfired = cr.check_conditions(case, outs, [cr.case_inputs(case, ls, n)[2] for n in range(3)])
    assert unfired > 0
    for f, rec in outs:
        assert cr.fragile(rec, kind).mean() <= cr.FRAGILE_SHARE[kind]
    keep = ~outs[2][1]["tropo_fired"] & outs[0][1]["tropo_fired"]
    assert keep.any() and np.array_equal(outs[2][0]["tropopause"][keep], outs[0][0]["tropopause"][keep])
    assert (outs[2][0]["tropopause"][keep] > 0).all()
    if ls == 1:
        o0 = restated(case, 0, kind) if (case, 0) in cr.RUNS else None
        if o0 is not None:          # the subgrid term only raises hmix, and changes nothing else
            assert (outs[0][0]["hmix"] >= o0[0][0]["hmix"]).all() and (outs[0][0]["hmix"] > o0[0][0]["hmix"]).any()
            for k in ("ustar", "wstar", "oli", "tropopause"):
                assert np.array_equal(outs[0][0][k], o0[0][0][k]), k


@pytest.fixture(scope="module")
def host_body(tmp_path_factory):
    d = tmp_path_factory.mktemp("cpg_host")
    exe = d / "calcpar_gfs_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(HERE, "calcpar_gfs_host.cpp"), "-o", str(exe)])
    return str(exe), d


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("run", cr.RUNS, ids=RUN_IDS)
def test_host_compiled_body_equals_reference_fixture(host_body, run, kind):
    """cpg::calcpar_gfs_column, the function the kernel calls per column, built with g++ -O2 -ffp-contract=off over glibc's
    libm: every field of every call bit for bit.  No column is handled by the margin rule."""
    case, ls = run
    exe, d = host_body
    mk = maker()
    fin, fout = str(d / f"in_{case}_{ls}_{kind}.bin"), str(d / f"out_{case}_{ls}_{kind}.bin")
    mk.write_input(fin, [cr.case_inputs(case, ls, n) for n in range(3)], mk.NCEP, ls)
    subprocess.check_call([exe, kind[1], fin, fout])
    kw = cr.CASES[case]
    g = golden(f"cpg_{case}", kind)
    for n, got in enumerate(mk.read_output(fout, 3, kw["ny"], kw["nx"])):
        for k in cr.FIELDS:
            want = g[f"{k}_{n}_ls{ls}"].astype(np.float64)
            assert np.array_equal(got[k], want), (n, k, int((got[k] != want).sum()))


@pytest.mark.ref
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_live_reference(kind, tmp_path):
    mk = maker()
    if not mk.available():
        pytest.skip("the reference tree and flang are not present")
    bd = os.path.join(ROOT, "oracle", "_ref", "cpgref")      # built once, outside git
    os.makedirs(bd, exist_ok=True)
    exe = mk.build(kind, bd)
    kw = dict(nx=40, ny=26, nz=30, terrain=21000.0)
    st = cr.new_state()
    calls, outs = [], []
    for slot, ph in zip((1, 2, 1), (3, 8, 1)):
        m = syn.gfs_levels(**kw, phase=ph)
        cin = syn.calcpar_gfs_inputs(m)
        calls.append((slot, m, cin))
        outs.append(cr.calcpar_gfs_ref(m, cin, kind, st, slot))
    refs = mk.run(exe, calls, mk.NCEP, 1, str(tmp_path))
    for n, (ref, (f, rec)) in enumerate(zip(refs, outs)):
        assert not rec["no_kzmin"].any()
        for k in cr.FIELDS:
            assert np.array_equal(ref[k], f[k]), (n, k)
    g = golden("cpg_flat", kind)                               # the committed fixture is what the reference gives
    refs = mk.run(exe, [cr.case_inputs("flat", 1, n) for n in range(3)], mk.NCEP, 1, str(tmp_path))
    for n, ref in enumerate(refs):
        for k in cr.FIELDS:
            assert np.array_equal(ref[k], g[f"{k}_{n}_ls1"].astype(np.float64)), (n, k)


@pytest.mark.parametrize("kind", KINDS)
def test_ecmwf_restatement_equals_the_unmodified_routine(kind):
    """The by-product of the stand-in module: oracle.cp_oracle (the C restatement of calcpar's ECMWF branch, "parity unpinned"
    until now) against the unmodified calcpar with metdata_format = GRIBFILE_CENTRE_ECMWF, bit for bit in ustar, oli, wstar,
    hmix on every column.  The tropopause is left out: calcpar.f90:232 starts its kzmin search at zlev(1), which the ECMWF
    branch never writes (:203 starts at 2), so the reference reads an undefined value there."""
    from oracle.oracle import cp_oracle
    mk = maker()
    m = syn.model_levels(**mk.ECMWF_CASE)
    o = cp_oracle(m, syn.calcpar_inputs(m), kind)
    g = golden("cp_ecmwf", kind)
    for k in ("ustar", "oli", "wstar", "hmix"):
        want = g[k].astype(np.float64)
        assert np.array_equal(o[k], want), (k, int((o[k] != want).sum()), np.argwhere(o[k] != want)[:5].tolist())


def test_abi_symbol_struct_and_fortran_interface(built, tmp_path):
    """The library exports fpx_calcpar_gfs, sizeof(fpx_calcpar_gfs_in) of the C header equals the ctypes mirror's, member by
    member in the same order, and the Fortran type and interface list the same members and arguments."""
    from flexpart_amd import _lib
    from flexpart_amd.engine import Engine
    lib = _lib.load()
    assert lib.fpx_abi_version() == 4
    assert "fpx_calcpar_gfs" in _lib.SYMBOLS and lib.fpx_calcpar_gfs is not None
    assert lib.fpx_calcpar_gfs.argtypes == [C.c_void_p, C.c_int32, C.POINTER(_lib.FpxCalcparGfsIn), C.POINTER(_lib.FpxCalcparOut)]
    assert callable(Engine.calcpar_gfs) and callable(syn.calcpar_gfs_inputs)
    names = [n for n, _ in _lib.FpxCalcparGfsIn._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flexpart_amd.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(fpx_calcpar_gfs_in));\n'
                   + "".join(f'  printf("{n} %zu\\n", offsetof(fpx_calcpar_gfs_in, {n}));\n' for n in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_lib.FpxCalcparGfsIn) == 2 * 4 + 5 * 8 + 2 * 4
    for n in names:
        assert int(got[n]) == getattr(_lib.FpxCalcparGfsIn, n).offset, n
    hdr = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    assert "int fpx_calcpar_gfs(fpx_handle h, int32_t slot, const fpx_calcpar_gfs_in *c, const fpx_calcpar_out *out);" in hdr
    f90 = open(os.path.join(ROOT, "flexpart_amd", "fortran", "flexgpu_mod.f90")).read()
    t = re.search(r"type, bind\(C\) :: fpx_calcpar_gfs_in\n(.*?)end type fpx_calcpar_gfs_in", f90, re.S).group(1)
    members = [v.strip() for line in t.strip().splitlines() for v in line.split("::")[1].split(",")]
    assert members == names
    i = re.search(r"function fpx_calcpar_gfs\(([^)]*)\) bind\(C, name='fpx_calcpar_gfs'\)\n(.*?)end function", f90, re.S)
    assert [a.strip() for a in i.group(1).split(",")] == ["h", "slot", "c", "o"]
    assert "type(fpx_calcpar_gfs_in), intent(in) :: c" in i.group(2) and "type(fpx_calcpar_out), intent(in) :: o" in i.group(2)
    assert "integer(c_int32_t), value :: slot" in i.group(2)
    assert re.search(r"subroutine flexgpu_calcpar_gfs\(n, ierr, writeback, device_vdep\)", f90)


# ---- GPU ---------------------------------------------------------------------------------------------------------
DROP = ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "uupol", "vvpol", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep")


def engine_for(m, kind, sc=None, **kw):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    nx, ny, nz = (int(v) for v in m["grid"])
    if sc is None:
        sc = syn.small(n=0, nx=nx, ny=ny, nz=nz, nsteps=1)
    sc = {k: v for k, v in dict(sc, grid=m["grid"], geom=m["geom"], globalflags=m["globalflags"]).items() if k not in DROP}
    rb = 8 if kind == "r8" else 4
    kw.setdefault("rng_mode", RNG_PHILOX)
    return Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, pad=(3, 2, 1), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("run", cr.RUNS, ids=RUN_IDS)
def test_device_matches_the_restatement(built, run, kind):
    """fpx_verttransform_gfs(sfc with NULL 2-D members) + fpx_calcpar_gfs over the three calls, against the restatement under
    the rule of tests/test_calcpar.py::test_device_calcpar_matches_the_restatement (the same arithmetic chain and device
    libm): 1e-10 (r8) / 2e-4 (r4) of the field's range; a column not within reach (1e-9 / 1e-4) of a threshold must agree
    without exception; ustar everywhere; at most 1 % of the columns off in the other fields."""
    case, ls = run
    want3 = restated(case, ls, kind)
    eng = engine_for(cr.case_inputs(case, ls, 0)[1], kind)
    got3 = []
    for n in range(3):
        slot, m, cin = cr.case_inputs(case, ls, n)
        eng.verttransform_gfs(slot, m, {}, init=(n == 0), want=())
        got3.append(eng.calcpar_gfs(slot, cin))
    eng.close()
    tol, reach = cr.TOL[kind], cr.REACH[kind]
    for n, (got, (want, rec)) in enumerate(zip(got3, want3)):
        ncol = want["hmix"].size
        fragile = rec["margin"] < reach
        assert fragile.mean() <= cr.FRAGILE_SHARE[kind], float(fragile.mean())
        for k in cr.FIELDS:
            assert np.isfinite(got[k]).all(), (n, k)
            scale = np.abs(want[k]).max()
            err = np.abs(got[k] - want[k])
            bad = err > tol * scale
            print(f"{case} ls={ls} {kind} call {n} {k}: worst {err[~fragile].max() / scale:.2e} outside reach, {int(bad.sum())} columns off, {int(fragile.sum())} fragile")
            assert not (bad & ~fragile).any(), (n, k, int((bad & ~fragile).sum()), float(err[~fragile].max() / scale))
            limit = 0 if k == "ustar" else 0.01 * ncol
            assert bad.sum() <= limit, (n, k, int(bad.sum()), float(err.max() / scale))
        assert got["device_ms"] > 0


def _two_fields(drydep, n=1500):
    """Two wind fields of `terrain` with their surface analysis, and n particles of syn.small on that grid."""
    kw = cr.CASES["terrain"]
    calls = [cr.case_inputs("terrain", 1, n) for n in range(2)]
    if drydep:
        from test_getvdep import particle_run
        sc, _ = particle_run(kw["nx"], kw["ny"], kw["nz"])
    else:
        sc = syn.small(n=n, nx=kw["nx"], ny=kw["ny"], nz=kw["nz"], nsteps=2, ctl=5.0, ifine=4)
    sc = dict(sc, ztra1=np.minimum(np.asarray(sc["ztra1"]), 5000.0))
    return calls, sc


def _fly(eng, sc):
    eng.set_windtime(sc["memtime"], sc["memind"])
    eng.upload_particles_from_scenario({k: v for k, v in sc.items() if k not in DROP})
    return eng.run(2)


@pytest.mark.gpu
@pytest.mark.parametrize("drydep", [False, True], ids=["plain", "drydep"])
def test_gather_packs_equal_the_upload_path(built, drydep):
    """Run B: verttransform_gfs(2-D members NULL) + calcpar_gfs per slot.  Run A: the arrays calcpar_gfs of run B returned go
    back in through the existing path, verttransform_gfs with a full sfc.  Both packs hold the same numbers, so 1500 particles
    stepped twice end on the same bits.  With DRYDEP run B computes vdep on the device (calcpar_gfs(device_vdep = 1), then
    fpx_getvdep from the ustar / oli left there) and run A uploads that vdep; and that vdep equals tests/getvdep_ref.py fed the
    restatement's ustar / oli under the rule of tests/test_getvdep.py."""
    from flexpart_amd.engine import RNG_TABLE_SEQ
    calls, sc = _two_fields(drydep)
    kw = cr.CASES["terrain"]
    tables = syn.getvdep_tables(kw["nx"], kw["ny"], 2) if drydep else None
    gins = [syn.getvdep_inputs(m, seed=4300 + 10 * s, wftime=10800 * s) for s, (_, m, _) in enumerate(calls)] if drydep else None
    engB = engine_for(calls[0][1], "r8", sc, rng_mode=RNG_TABLE_SEQ)
    if drydep:
        engB.getvdep_init(tables)
    sfcs = []
    for s, (slot, m, cin) in enumerate(calls):
        engB.verttransform_gfs(slot, m, {}, init=(s == 0), want=())
        out = engB.calcpar_gfs(slot, cin, device_vdep=drydep)
        sfc = {k: out[k] for k in cr.FIELDS}
        if drydep:
            sfc["vdep"] = engB.getvdep(slot, gins[s])["vdep"]
        sfcs.append(sfc)
    gotB = _fly(engB, sc)
    engB.close()
    engA = engine_for(calls[0][1], "r8", sc, rng_mode=RNG_TABLE_SEQ)
    for s, (slot, m, cin) in enumerate(calls):
        engA.verttransform_gfs(slot, m, sfcs[s], init=(s == 0), want=())
    gotA = _fly(engA, sc)
    engA.close()
    assert np.abs(gotB[-1]["xtra1"] - np.asarray(sc["xtra1"])).max() > 0        # the particles moved
    for a, b in zip(gotA, gotB):
        for k in ("xtra1", "ytra1", "ztra1", "xmass1"):
            assert np.array_equal(a[k], b[k]), k
    if drydep:
        import getvdep_ref as gr
        import test_getvdep as tg
        want3 = restated("terrain", 1, "r8")
        for s, (slot, m, cin) in enumerate(calls):
            full = dict(gins[s], ustar=want3[s][0]["ustar"], oli=want3[s][0]["oli"], ps=m["ps"], tt2=m["tt2"], td2=m["td2"])
            want = gr.getvdep_ref(tables, full, float(m["geom"][1]), float(m["geom"][3]), "r8")
            frag = tg.fragile("r8", want)
            assert frag.mean() <= 0.0
            w = tg.worst(sfcs[s]["vdep"], want["vdep"])
            print(f"getvdep after calcpar_gfs, slot {slot}: max relative deviation {w.max():.3e}")
            assert w[~frag].max() <= tg.TOL["r8"], float(w[~frag].max())


@pytest.mark.gpu
def test_step_refuses_a_slot_whose_boundary_layer_fields_are_stale(built):
    """fpx_verttransform_gfs with the 2-D members NULL promises that fpx_calcpar_gfs follows: after the next wind field's
    transform and before its calcpar_gfs the step returns FPX_ERR_STATE; after it, it runs."""
    from flexpart_amd.engine import RNG_TABLE_SEQ
    from flexpart_amd._lib import FpxError
    calls, sc = _two_fields(False, n=200)
    third = cr.case_inputs("terrain", 1, 2)
    eng = engine_for(calls[0][1], "r8", sc, rng_mode=RNG_TABLE_SEQ)
    for s, (slot, m, cin) in enumerate(calls):
        eng.verttransform_gfs(slot, m, {}, init=(s == 0), want=())
        eng.calcpar_gfs(slot, cin)
    eng.set_windtime(sc["memtime"], sc["memind"])
    eng.upload_particles_from_scenario({k: v for k, v in sc.items() if k not in DROP})
    eng.step(0)
    eng.verttransform_gfs(1, third[1], {}, want=())             # next wind field into slot 1, calcpar_gfs forgotten
    with pytest.raises(FpxError) as e:
        eng.step(900)
    assert e.value.code == -3 and "field slots" in str(e.value), str(e.value)
    eng.calcpar_gfs(1, third[2])
    eng.step(900)
    eng.close()


@pytest.mark.gpu
def test_refusals(built):
    from flexpart_amd._lib import FpxError
    UNSUPPORTED, ARG, STATE = -5, -1, -3
    slot, m, cin = cr.case_inputs("flat", 1, 0)
    nx, ny = cr.CASES["flat"]["nx"], cr.CASES["flat"]["ny"]
    full = {k: np.full((ny, nx), v) for k, v in (("hmix", 800.0), ("ustar", 0.3), ("wstar", 1.0), ("oli", 0.01), ("tropopause", 11000.0))}

    def refused(fn, code, *words):
        with pytest.raises(FpxError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for wd in words:
            assert wd in str(e.value), str(e.value)

    eng = engine_for(m, "r8")
    refused(lambda: eng.calcpar_gfs(1, cin), UNSUPPORTED, "GFS")                                  # no transform yet: not a GFS handle
    refused(lambda: eng.verttransform_gfs(1, m, {"hmix": full["hmix"]}, init=True), ARG, "all five NULL")
    refused(lambda: eng.verttransform_gfs(1, m, {k: full[k] for k in ("ustar", "wstar", "oli", "tropopause")}, init=True), ARG, "hmix")
    eng.verttransform_gfs(1, m, {}, init=True, want=())
    refused(lambda: eng.calcpar_gfs(2, cin), STATE, "fpx_verttransform_gfs of this slot first")   # the wrong slot
    refused(lambda: eng.calcpar_gfs(1, dict(cin, hmix=None)), ARG, "hmix")
    refused(lambda: eng.calcpar_gfs(1, dict(cin, excessoro=None)), ARG, "excessoro")
    eng.calcpar_gfs(1, dict(cin, excessoro=None, lsubgrid=0))
    eng.close()
    me = syn.model_levels(nx=nx, ny=ny, nz=cr.CASES["flat"]["nz"], global_grid=False)
    eng = engine_for(me, "r8")
    eng.verttransform(1, me, None, init=True, want=())
    refused(lambda: eng.calcpar_gfs(1, cin), UNSUPPORTED, "GFS", "fpx_calcpar")                   # an ECMWF handle
    eng.close()
