"""verttransform_gfs (NCEP GFS fields on pressure levels): restatement vs the reference (CPU), HIP path vs both (GPU).

CPU (-m "not gpu"): the numpy restatement tests/verttransform_gfs_ref.py equals bit for bit what the unmodified routine left
in com_mod (tests/golden/vtgfs_<case>_<kind>.npz, flang build driven by tests/golden/ref_vg_driver.f90) after each of the
three calls of a case -- slot 1 with init, slot 2, slot 1 again with another phase, the call that shows the ww the slot
carries (verttransform_gfs.f90:271-285,354).  A fixture holds the SHA-256 of every array of every call and the arrays
themselves as far as the size limit of a committed file allows (make_vtgfs_golden.py says which): the digests carry the
bit-for-bit comparison, the stored arrays are compared element by element as well.  ww is compared outside the mask (the
cells whose slope term reads an entry of the automatic array uvwzlev that the routine never wrote: NaN in the restatement).
`cap` has no z level above hmixmax, so the reference leaves nmixz unset there (:126-131); restatement and engine say nz.

GPU (-m gpu): fpx_verttransform_gfs through the C ABI.  Bounds are those of tests/test_verttransform.py -- 1e-11 (f64) and
1e-4 (f32) of each field's range -- with the same exposure: log in the height recursion, cos / sin / atan at the caps."""
import ctypes as C
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import verttransform_gfs_ref as vr
from flexpart_amd import synthetic as syn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ["r8", "r4"]
TOL = {"r8": 1e-11, "r4": 1e-4}
OUT3 = ("uu", "vv", "ww", "tt", "qv", "pv", "rho", "drhodz", "pplev", "uupol", "vvpol")
PAD = (3, 2, 1)
_cache = {}


def restated(case, kind):
    """The three calls of a case in the restatement, computed once and shared: [(fields, rec)] * 3."""
    if (case, kind) not in _cache:
        kw = vr.CASES[case]
        _cache[(case, kind)] = vr.run_case(kw, vr.PHASES, kind, vr.case_polemaps(kw, kind))
    return _cache[(case, kind)]


def golden(case, kind):
    if ("gold", case, kind) not in _cache:
        _cache[("gold", case, kind)] = np.load(os.path.join(GOLD, f"vtgfs_{case}_{kind}.npz"))
    return _cache[("gold", case, kind)]


def maker():
    spec = importlib.util.spec_from_file_location("make_vtgfs_golden", os.path.join(GOLD, "make_vtgfs_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rows_of(case):
    return vr.polar_rows(syn.gfs_levels(**vr.CASES[case]))


def comparable(field, a, mask, rows):
    if field == "ww":
        return np.where(mask, 0.0, a)
    if field in ("uupol", "vvpol"):
        return a[:, rows, :]
    return a


def sha(a, kind):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a.astype(vr.KINDS[kind])).tobytes()).digest(), np.uint8)


# ---- CPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(vr.CASES))
def test_restatement_equals_reference_fixture(case, kind):
    g = golden(case, kind)
    rows = rows_of(case)
    levels = list(maker().LEVELS_KEPT)
    outs = restated(case, kind)
    assert np.array_equal(outs[0][0]["height"], g["height"])
    if (g["height"] > 4500.0).any():
        assert outs[0][0]["nmixz"] == int(g["nmixz"])
    for n, (f, rec) in enumerate(outs):
        mask = np.isnan(f["ww"])
        for k in OUT3:
            if k in ("uupol", "vvpol") and not rows.any():
                continue
            a = comparable(k, f[k], mask, rows)
            assert np.isfinite(a).all(), (n, k)
            if f"{k}_{n}" in g.files:
                stored = g[f"{k}_{n}"].astype(np.float64)
                part = a if stored.shape == a.shape else a[levels]
                assert np.array_equal(part, stored), (n, k, float(np.abs(part - stored).max()))
            assert np.array_equal(sha(a, kind), g[f"sha_{n}_{k}"]), (n, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(vr.CASES))
def test_inputs_meet_the_conditions(case, kind):
    """The conditions on the synthetic inputs, again from the restatement's record (the fixture script asserts them before it
    writes): masked cells, branch counters, the cap of llev, no slope bracket carried across columns, the margin of every
    above-the-top decision.  And the third call really shows the carried ww: its cells above a column's top differ from what
    a fresh slot would give."""
    kw = vr.CASES[case]
    outs = restated(case, kind)
    vr.check_conditions(case, kw, outs)
    if case != "flat":
        st = vr.new_state()
        st["height"], st["nmixz"] = vr.KINDS[kind](outs[0][0]["height"]), outs[0][0]["nmixz"]
        fresh, _ = vr.vtgfs_ref(syn.gfs_levels(**kw, phase=vr.PHASES[2]), kind, st, 1, polemaps=vr.case_polemaps(kw, kind))
        with np.errstate(invalid="ignore"):
            differ = (fresh["ww"] != outs[2][0]["ww"]) & ~np.isnan(fresh["ww"])
        assert differ.any()
        for k in ("uu", "rho", "pplev", "drhodz"):
            assert np.array_equal(fresh[k], outs[2][0][k]), k


@pytest.mark.ref
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_live_reference(kind, tmp_path):
    mk = maker()
    if not mk.available():
        pytest.skip("the reference tree and flang are not present")
    kw = dict(vr.CASES["terrain"], nx=44, ny=18)
    phases = (2, 7, 5)
    pm = vr.case_polemaps(kw, kind)
    outs = vr.run_case(kw, phases, kind, pm)
    bd = os.path.join(os.path.dirname(os.path.dirname(GOLD)), "oracle", "_ref", "vgref")      # built once, outside git
    os.makedirs(bd, exist_ok=True)
    exe = mk.build(kind, bd)
    refs = mk.run(exe, [(slot, syn.gfs_levels(**kw, phase=ph)) for slot, ph in zip((1, 2, 1), phases)], str(tmp_path))
    rows = vr.polar_rows(syn.gfs_levels(**kw))
    for n, (ref, (f, rec)) in enumerate(zip(refs, outs)):
        assert rec["carry_across"] == 0
        mask = np.isnan(f["ww"])
        assert np.array_equal(ref["height"], f["height"]) and ref["nmixz"] == f["nmixz"]
        for k in OUT3:
            assert np.array_equal(comparable(k, ref[k], mask, rows), comparable(k, f[k], mask, rows)), (n, k)


def test_abi_version_symbol_and_prototype(built):
    from flexpart_amd import _lib
    lib = _lib.load()
    assert lib.fpx_abi_version() == 4
    assert "fpx_verttransform_gfs" in _lib.SYMBOLS and lib.fpx_verttransform_gfs is not None
    assert lib.fpx_verttransform_gfs.argtypes == [C.c_void_p, C.c_int32, C.POINTER(_lib.FpxModelLevels), C.POINTER(_lib.FpxFields),
                                                  C.POINTER(_lib.FpxFieldsOut), C.c_void_p]
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "flexpart_amd.h")).read()
    assert ("int fpx_verttransform_gfs(fpx_handle h, int32_t slot, const fpx_model_levels *m, const fpx_fields *sfc, "
            "const fpx_fields_out *out, void *pplev_out);") in hdr
    from flexpart_amd.engine import Engine
    assert callable(Engine.verttransform_gfs)


# ---- GPU ---------------------------------------------------------------------------------------------------------
def engine_for(m, kind, sc=None, pad=PAD):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    nx, ny, nz = (int(v) for v in m["grid"])
    drop = ("height", "nmixz", "uu", "vv", "ww", "rho", "drhodz", "tt", "uupol", "vvpol", "hmix", "ustar", "wstar", "oli", "tropopause", "vdep")
    if sc is None:
        sc = syn.small(n=0, nx=nx, ny=ny, nz=nz, nsteps=1)
    sc = {k: v for k, v in dict(sc, grid=m["grid"], geom=m["geom"], globalflags=m["globalflags"]).items() if k not in drop}
    rb = 8 if kind == "r8" else 4
    return Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=RNG_PHILOX, pad=pad)


def sfc_for(nx, ny, n=0):
    return {k: np.full((ny, nx), v) for k, v in (("hmix", 800.0 + 50.0 * n), ("ustar", 0.3), ("wstar", 1.0), ("oli", 0.01), ("tropopause", 11000.0))}


def device(case, kind):
    """The three calls of a case on the device, run once and shared."""
    if ("dev", case, kind) not in _cache:
        kw = vr.CASES[case]
        ms = [syn.gfs_levels(**kw, phase=ph) for ph in vr.PHASES]
        eng = engine_for(ms[0], kind)
        outs = [eng.verttransform_gfs(slot, m, sfc_for(kw["nx"], kw["ny"], n), init=(n == 0)) for n, (slot, m) in enumerate(zip((1, 2, 1), ms))]
        eng.close()
        _cache[("dev", case, kind)] = outs
    return _cache[("dev", case, kind)]


def worst_rel(got, want, mask, rows):
    worst = {}
    for k in OUT3:
        if k in ("uupol", "vvpol") and not rows.any():
            continue
        a, b = comparable(k, got[k], mask, rows), comparable(k, want[k], mask, rows)
        worst[k] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    worst["height"] = float(np.abs(got["height"] - want["height"]).max() / np.abs(want["height"]).max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(vr.CASES))
def test_hip_matches_restatement(built, case, kind):
    """All cases, both kinds, all three calls; plus what must be exact: nmixz, and the cells that are pure copies -- z level 1
    and nz of uu, vv, tt, qv, pv (model levels llev and nuvz) and pplev(1) = akz(llev)."""
    rows = rows_of(case)
    kw = vr.CASES[case]
    H = vr.KINDS[kind]
    for n, (got, (want, rec)) in enumerate(zip(device(case, kind), restated(case, kind))):
        assert got["nmixz"] == want["nmixz"]
        mask = np.isnan(want["ww"])
        for k in OUT3:
            assert np.isfinite(got[k]).all(), (n, k)
        worst = worst_rel(got, want, mask, rows)
        print(f"{case} {kind} call {n}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert max(worst.values()) <= TOL[kind], (n, worst)
        m = syn.gfs_levels(**kw, phase=vr.PHASES[n])
        for k, src in (("uu", "uuh"), ("vv", "vvh"), ("tt", "tth"), ("qv", "qvh"), ("pv", "pvh")):
            a = np.asarray(m[src]).astype(H).astype(np.float64)
            assert np.array_equal(got[k][0], np.take_along_axis(a, (rec["llev"] - 1)[None], 0)[0]), (n, k)
            assert np.array_equal(got[k][-1], a[-1]), (n, k)
            assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][-1], want[k][-1]), (n, k)
        akz = np.asarray(m["akz"]).astype(H).astype(np.float64)
        assert np.array_equal(got["pplev"][0], akz[rec["llev"] - 1]) and (got["pplev"][-1] == akz[-1]).all(), n


@pytest.mark.gpu
def test_hip_against_reference_fixture(built):
    """f64 `terrain` directly against the unmodified routine's output, no restatement in between (its record only says which
    ww cells are masked): every array the fixture stores, of every call."""
    case, kind = "terrain", "r8"
    g = golden(case, kind)
    rows = rows_of(case)
    levels = list(maker().LEVELS_KEPT)
    seen = 0
    for n, (got, (want, rec)) in enumerate(zip(device(case, kind), restated(case, kind))):
        mask = np.isnan(want["ww"])
        for k in OUT3:
            if f"{k}_{n}" not in g.files:
                continue
            stored = g[f"{k}_{n}"].astype(np.float64)
            a = comparable(k, got[k], mask, rows)
            part = a if stored.shape == a.shape else a[levels]
            err = float(np.abs(part - stored).max() / np.abs(stored).max())
            assert err <= TOL[kind], (n, k, err)
            seen += 1
    assert seen == 3 + 10          # ww of every call, the other ten fields of the third
    assert got["nmixz"] == int(g["nmixz"])
    assert np.abs(got["height"] - g["height"]).max() <= TOL[kind] * np.abs(g["height"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_device_pv_on_gfs_input(built, kind):
    """pvh = NULL: fpx_get_pvh equals calcpv_ref on the GFS input within the bound of tests/test_calcpv.py (its rule: every
    point within TOL, points within REACH of another path counted and capped), and the transform's pv follows it."""
    import calcpv_ref as pr
    import test_calcpv as tp
    kw = vr.CASES["terrain"]
    m = syn.gfs_levels(**kw)
    r = pr.calcpv_ref(m, kind)
    eng = engine_for(m, kind)
    given = eng.verttransform_gfs(1, m, sfc_for(kw["nx"], kw["ny"]), init=True, want=("pv",))
    out = eng.verttransform_gfs(1, m, sfc_for(kw["nx"], kw["ny"]), want=("pv",), device_pv=True)
    got = eng.get_pvh()
    eng.close()
    assert given["calcpv_ms"] == 0.0 and out["calcpv_ms"] > 0 and out["device_ms"] > 0
    frag = r["margin"] < tp.REACH[kind]
    e = pr.level_error(got, r["pvh"])
    bad = e > tp.TOL[kind]
    print(f"device calcpv on GFS input {kind}: worst {e[~frag].max():.3e} outside reach, {int(frag.sum())} fragile points of {frag.size}, "
          f"{int((bad & frag).sum())} of them beyond the tolerance")
    assert np.isfinite(got).all()
    assert not (bad & ~frag).any(), float(e[~frag].max())
    assert (bad & frag).sum() <= tp.CAP[kind] * frag.size
    assert not np.array_equal(out["pv"], given["pv"])
    # the z-level pv is the transform of the device's pvh: level 1 and nz are copies of model levels llev and nuvz
    llev = vr.llev_of(np.asarray(m["ps"]).astype(vr.KINDS[kind]), np.asarray(m["akz"]).astype(vr.KINDS[kind]))
    assert np.array_equal(out["pv"][0], np.take_along_axis(got, (llev - 1)[None], 0)[0]) and np.array_equal(out["pv"][-1], got[-1])


@pytest.mark.gpu
def test_trajectories_on_device_transformed_gfs_fields(built):
    """As test_trajectories_on_device_transformed_fields: a few thousand particles stepped on fields the device transformed
    itself equal the same particles stepped on the restatement's fields given through fpx_upload_fields."""
    from flexpart_amd.engine import Engine, RNG_TABLE_SEQ
    from test_gpu_parity import assert_close
    nx, ny, nz = 40, 24, 16
    kw = dict(nx=nx, ny=ny, nz=nz, global_grid=True, polar=False, terrain=0.0)
    ms = [syn.gfs_levels(**kw, phase=p) for p in (0, 6)]
    st = vr.new_state()
    w = [vr.vtgfs_ref(ms[s], "r8", st, s + 1, init=(s == 0)) for s in (0, 1)]
    assert w[0][1]["masked"] == 0 and w[1][1]["masked"] == 0
    sc = dict(syn.small(n=3000, nx=nx, ny=ny, nz=nz, nsteps=3, ctl=5.0, ifine=4))
    sc["height"] = w[0][0]["height"]; sc["nmixz"] = w[0][0]["nmixz"]
    for k in ("uu", "vv", "ww", "rho", "drhodz", "tt"):
        sc[k] = np.stack([w[0][0][k], w[1][0][k]])
    sc.update(syn.make_particles(3000, nx, ny, sc["height"], sc["hmix"], seed=11))
    ref = Engine(sc, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_TABLE_SEQ)
    want = ref.run(3)
    ref.close()
    sc_e = {k: v for k, v in sc.items() if k not in ("uu", "vv", "ww", "rho", "drhodz", "tt", "height", "nmixz")}
    eng = Engine(sc_e, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_TABLE_SEQ)
    for slot in (0, 1):
        sfc = {k: sc[k][slot] for k in ("hmix", "ustar", "wstar", "oli", "tropopause")}
        eng.verttransform_gfs(slot + 1, ms[slot], sfc, init=(slot == 0), want=())
    eng.set_windtime(sc["memtime"], sc["memind"])
    got = eng.run(3)
    eng.close()
    assert np.abs(want[-1]["xtra1"] - sc["xtra1"]).max() > 0        # the particles moved
    for g, wv in zip(got, want):
        assert_close(g, wv, 1e-8, 1e-6)


@pytest.mark.gpu
def test_refusals(built):
    """Each refusal returns its error with a message that names what differs."""
    from flexpart_amd import _lib
    from flexpart_amd._lib import FpxError
    kw = vr.CASES["cap"]
    nx, ny = kw["nx"], kw["ny"]
    m = syn.gfs_levels(**kw)
    UNSUPPORTED, ARG = -5, -1

    def refused(fn, code, *words):
        with pytest.raises(FpxError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for wd in words:
            assert wd in str(e.value), str(e.value)

    eng = engine_for(m, "r8")
    refused(lambda: eng.verttransform_gfs(1, m, None, init=True), UNSUPPORTED, "sfc", "calcpar.f90:109-121,145-149")
    refused(lambda: eng.verttransform_gfs(1, dict(m, nuvz=kw["nz"] - 1), sfc_for(nx, ny), init=True), ARG, "nuvz")
    eng.verttransform_gfs(1, m, sfc_for(nx, ny), init=True, want=())
    lib = eng.lib
    refused(lambda: _lib.check(lib.fpx_calcpar(eng.h, 1, C.byref(_lib.FpxCalcparIn()), None), "fpx_calcpar"), UNSUPPORTED, "calcpar.f90:109-121,145-149")
    refused(lambda: _lib.check(lib.fpx_calcpar_nest(eng.h, 1, 1, C.byref(_lib.FpxCalcparIn()), None), "fpx_calcpar_nest"), UNSUPPORTED, "calcpar.f90:109-121,145-149")
    refused(lambda: _lib.check(lib.fpx_conv_init(eng.h, C.byref(_lib.FpxConvConfig())), "fpx_conv_init"), UNSUPPORTED,
            "convmix.f90:100-116,173-189", "calcmatrix.f90")
    refused(lambda: _lib.check(lib.fpx_convmix(eng.h, 0, None), "fpx_convmix"), UNSUPPORTED, "convmix.f90:100-116,173-189", "calcmatrix.f90")
    me = syn.model_levels(nx=nx, ny=ny, nz=kw["nz"], global_grid=False)
    refused(lambda: eng.verttransform(1, me, sfc_for(nx, ny)), UNSUPPORTED, "GFS")
    refused(lambda: _lib.check(lib.fpx_verttransform_nest(eng.h, 1, 1, C.byref(_lib.FpxModelLevels()), None, C.byref(_lib.FpxFieldsOut())),
                               "fpx_verttransform_nest"), UNSUPPORTED, "GFS")
    eng.close()
    eng = engine_for(me, "r8")
    eng.verttransform(1, me, sfc_for(nx, ny), init=True, want=())
    refused(lambda: eng.verttransform_gfs(1, m, sfc_for(nx, ny)), UNSUPPORTED, "ECMWF")
    eng.close()
