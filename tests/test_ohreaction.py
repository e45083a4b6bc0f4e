"""OH chemistry: fpx_oh_init, fpx_gethourlyOH, fpx_ohreaction, fpx_get_oh_hourly, fpx_set_oh_hourly, fpx_ohreaction_time.
Reference: gethourlyOH.f90:40-142 (called at timemanager.f90:212-216) with zenithangle.f90, photo_O1D.f90, caldate.f90, and
ohreaction.f90:47-153 (called at timemanager.f90:171-172).

CPU: the numpy restatement tests/ohreaction_ref.py and the host-compiled bodies (tests/ohreaction_host.cpp around
flexpart_amd/csrc/fpx_ohreaction.hpp) against what flang builds of the unmodified routines leave behind after each call of
flexpart_amd.synthetic.oh_case() in both run directions (tests/golden/oh_r4.npz, oh_r8.npz), the conditions the case must
offer, and the refusal of an axis the nearest-index search cannot bisect.
GPU: the C ABI against the same fixtures.

THE RULE.  gethourlyOH runs on the host side with libm in the reference's order: OH_hourly and memOHtime are EQUAL.  In
ohreaction every index and the blended OH are exact IEEE arithmetic, so the CPU sides are EQUAL to the fixtures in every mass,
and on the device only pow and two exp differ from libm.  There the masses of species 2, of the particles in dark or empty OH
cells, of dead spaces and of the two zeroed particles are EQUAL; every other mass obeys a per-particle bound derived at test
time (device_bound): with x = ohrate |ltsample|,
    |got - want| <= want * (expm1(x * rho) + d_exp + eps),   rho = d_pow + d_exp + 4 eps,
where d_f = 2 * (worst relative error of the device's f over the arguments of the case, measured through fpx_math_probe
against mpmath or numpy.longdouble) + eps (libm's 1 ulp on the reference side), 4 eps the roundings of the three products of
ohrate and of x on both sides, and the last eps those of the final product.  tt and OH differ between neighbouring cells by
more than 2.7 % and 0.1 % (the maker asserts it), so one index off by one breaks the bound by orders of magnitude."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ohreaction_ref as oref
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ("r4", "r8")
TAG = {1: "f", -1: "b"}
sys.path.insert(0, GOLD)


@pytest.fixture(scope="module")
def gold():
    return {k: np.load(os.path.join(GOLD, f"oh_{k}.npz")) for k in KINDS}


@pytest.fixture(scope="module")
def restated():
    """run_case() of the restatement per kind and direction: computed once, never modified."""
    out = {}
    for ld in syn.OH_DIRECTIONS:
        c = syn.oh_case(ld)
        for kind in KINDS:
            out[kind, ld] = (c,) + oref.run_case(c, kind, syn.oh_masses(c, kind))
    return out


def gold_calls(g, c):
    tag = TAG[int(c["ldirect"])]
    return [dict(OH_hourly=g[f"{tag}_OH_hourly_{i}"], memOHtime=g[f"{tag}_memOHtime_{i}"]) if call[0] == "hourly" else dict(xmass1=g[f"{tag}_xmass1_{i}"])
            for i, call in enumerate(c["calls"])]


# ---- CPU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ld", syn.OH_DIRECTIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(restated, gold, kind, ld):
    """OH_hourly, memOHtime and xmass1 of every call, bit for bit, in both real kinds (all storage spaces: the restatement
    runs over the dead ones as the reference does)."""
    c, res, _ = restated[kind, ld]
    want = gold_calls(gold[kind], c)
    assert len(res) == len(want) == 5
    for r, w in zip(res, want):
        for k, v in w.items():
            assert v.dtype == oref.RT[kind] and r[k].dtype == oref.RT[kind]
            assert np.array_equal(r[k], v), (k, int((r[k] != v).sum()))


@pytest.mark.parametrize("ld", syn.OH_DIRECTIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_case_offers_every_branch_with_a_margin(kind, ld):
    """What the golden maker asserts before it writes: no particle without a level above it, no nearest-index tie, nothing
    outside, every branch of gethourlyOH, both outcomes of both tiny tests, the slot quirk, at most 10 % dead spaces, ..."""
    import make_ohreaction_golden as mk
    mk.check_conditions(syn.oh_case(ld), kind)


@pytest.fixture(scope="module")
def host_body(tmp_path_factory):
    d = tmp_path_factory.mktemp("oh_host")
    exe = d / "ohreaction_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(HERE, "ohreaction_host.cpp"), "-o", str(exe)])
    return str(exe), d


@pytest.mark.parametrize("ld", syn.OH_DIRECTIONS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_compiled_bodies_reproduce_the_reference(host_body, gold, restated, kind, ld):
    """oh::Hourly (gethourlyOH on the engine's host side) and oh_particle / the blend of fpx_ohreaction.hpp as host code:
    OH_hourly and memOHtime of every call and xmass1 of the live spaces bit for bit; the dead spaces keep their masses."""
    import make_ohreaction_golden as mk
    exe, d = host_body
    c, res, _ = restated[kind, ld]
    fin, fout, fdead = (str(d / f"{n}_{kind}_{ld}.bin") for n in ("in", "out", "itra1"))
    mk.write_input(c, kind, fin)
    np.asarray(c["itra1"], np.int32).tofile(fdead)
    text = subprocess.check_output([exe, kind[1], fin, fout, fdead], text=True).split()
    assert text == ["branch", "2", "skipped", "0", "branch", "1", "branch", "0", "skipped", "0"]
    want = gold_calls(gold[kind], c)
    live = np.asarray(c["itra1"]) != oref.DEAD
    m0 = syn.oh_masses(c, kind)
    nxo, nyo, nzo = (int(v) for v in c["ohgrid"])
    n = int(c["npart"])
    with open(fout, "rb") as f:
        for call, w in zip(c["calls"], want):
            if call[0] == "hourly":
                assert np.array_equal(np.fromfile(f, np.float64, 2).astype(oref.RT[kind]), w["memOHtime"])
                assert np.array_equal(np.fromfile(f, np.float64, 2 * nzo * nyo * nxo).reshape(2, nzo, nyo, nxo).astype(oref.RT[kind]), w["OH_hourly"])
            else:
                m = np.fromfile(f, np.float64, 3 * n).reshape(3, n).astype(oref.RT[kind])
                assert np.array_equal(m[:, live], w["xmass1"][:, live])
                assert np.array_equal(m[:, ~live], m0[:, ~live])


@pytest.mark.parametrize("rb", (4, 8))
def test_axis_check_refuses_what_the_search_cannot_bisect(host_body, rb):
    """oh::check_axis, the check of fpx_oh_init on lonOH, latOH and altOHtop: strictly increasing, every spacing above four
    units in the last place of the largest magnitude."""
    exe, _ = host_body
    ask = lambda *v: subprocess.check_output([exe, "axis", str(rb)] + [repr(float(x)) for x in v], text=True).strip()
    assert ask(-180., -135., 0., 180.) == "ok"
    assert "does not increase strictly" in ask(0., 10., 10., 20.)
    assert "does not increase strictly" in ask(0., 20., 10.)
    ulp = float(np.spacing(oref.RT["r4" if rb == 4 else "r8"](1024.)))
    assert "four units in the last place" in ask(0., 1024. - 4. * ulp, 1024.)
    assert ask(0., 1024. - 16. * ulp, 1024.) == "ok"
    assert "not finite" in ask(0., float("inf"))


def test_header_cites_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    for name in ("fpx_oh_init", "fpx_gethourlyOH", "fpx_ohreaction", "fpx_get_oh_hourly", "fpx_set_oh_hourly", "fpx_ohreaction_time",
                 "timemanager.f90:212-216", "timemanager.f90:171-172", "gethourlyOH.f90:40-142", "ohreaction.f90:47-153", "FLEXPART.f90:348-353"):
        assert name in text, name


def test_library_exports_the_new_symbols(built):
    from flexpart_amd import _lib
    lib = _lib.load()
    for n in ("fpx_oh_init", "fpx_gethourlyOH", "fpx_ohreaction", "fpx_get_oh_hourly", "fpx_set_oh_hourly", "fpx_ohreaction_time"):
        assert hasattr(lib, n), n
    assert lib.fpx_abi_version() == 4
    assert _lib.SYMBOLS_MIXED_CASE == ["fpx_gethourlyOH"]


# ---- GPU ------------------------------------------------------------------------------------------------------

ENGINES = [(8, 8), (4, 4)]          # (compute_real_bytes, host_real_bytes): fp64 engine with an r8 host, f32 engine with an r4 host
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


def kind_of(hb):
    return "r4" if hb == 4 else "r8"


def base_scenario(c, n=None):
    """syn.small on the grid of the case, with the case's geometry and its particles (or the first / last n of them)."""
    nx, ny, nz = (int(v) for v in c["grid"])
    sc = syn.small(n=8, nx=nx, ny=ny, nz=nz, nspec=3, global_grid=False, ldirect=int(c["ldirect"]), nsteps=1)
    sc["geom"] = np.asarray(c["geom"], np.float64)
    assert np.array_equal(sc["height"], c["height"])
    return sc


def particles(c, kind, sel=slice(None)):
    m = syn.oh_masses(c, kind)[:, sel]
    n = m.shape[1]
    return dict(npart=n, xtra1=c["xtra1"][sel], ytra1=c["ytra1"][sel], ztra1=c["ztra1"][sel], itra1=c["itra1"][sel], xmass1=m,
                itramem=np.zeros(n, np.int32), idt=np.full(n, 900, np.int32), npoint=np.ones(n, np.int32), nclass=np.ones(n, np.int32),
                itrasplit=np.full(n, 999999999, np.int32), cbt=np.ones(n, np.int16),
                **{k: np.zeros(n) for k in ("uap", "ucp", "uzp", "us", "vs", "ws")})


def make_engine(c, cb, hb, sel=slice(None), oh=True, nest=True, tt_slots=(1, 2)):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    eng = Engine(base_scenario(c), compute_real_bytes=cb, host_real_bytes=hb, rng_mode=RNG_PHILOX, seed=4711, max_particles=int(c["npart"]), pad=syn.OH_PAD)
    eng.upload_particles_from_scenario(particles(c, kind_of(hb), sel))
    if nest:
        eng.init_nest(c["nest"], c["nestgeom"])
    if tt_slots:
        eng.upload_tt(c["tt"], tt_slots)
    if oh:
        eng.oh_init(c)
    return eng


def run_calls(eng, c, calls=None, reset_to=None):
    """The calls of the case on the engine -> per call (OH_hourly, memOHtime, branch) | xmass1 [3][n] by particle number.
    reset_to: per call index the masses to upload before that ohreaction (the fixture's, so that errors do not accumulate)."""
    out = []
    for i, call in enumerate(c["calls"] if calls is None else calls):
        if call[0] == "hourly":
            br = eng.gethourlyOH(call[1])
            out.append(eng.get_oh_hourly() + (br,))
        else:
            _, itime, lts, mt, mi = call
            if reset_to and i in reset_to:
                p = particles(c, "r8")
                p["xmass1"] = reset_to[i]
                eng.upload_particles_from_scenario(p)
            eng.set_windtime(mt, mi)
            eng.ohreaction(itime, lts)
            out.append(eng.download()["xmass1"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ld", syn.OH_DIRECTIONS)
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_gethourlyOH_equals_the_reference(built, gold, cb, hb, ld):
    """fpx_gethourlyOH: the init branch, the advance at the hour, nothing inside it: OH_hourly and memOHtime bit for bit."""
    kind = kind_of(hb)
    c = syn.oh_case(ld)
    eng = make_engine(c, cb, hb)
    want = gold_calls(gold[kind], c)
    hourly = [(i, call) for i, call in enumerate(c["calls"]) if call[0] == "hourly"]
    branches = []
    for (i, call), got in zip(hourly, run_calls(eng, c, [call for _, call in hourly])):
        assert got[0].dtype == oref.RT[kind]
        assert np.array_equal(got[0], want[i]["OH_hourly"]), (i, int((got[0] != want[i]["OH_hourly"]).sum()))
        assert np.array_equal(got[1], want[i]["memOHtime"])
        branches.append(got[2])
    assert branches == [oref.BR_INIT, oref.BR_ADVANCE, oref.BR_NONE]
    eng.close()


def _truth(fn, x, y=None, single=False):
    """exp(x) or pow(x, y) far beyond the working precision: numpy.longdouble for f32 arguments, mpmath for f64."""
    if single:
        x = np.asarray(x, np.float32).astype(np.longdouble)
        return np.exp(x) if fn == "exp" else np.power(x, np.asarray(y, np.float32).astype(np.longdouble))
    import mpmath
    mpmath.mp.dps = 50
    if fn == "exp":
        return [mpmath.exp(mpmath.mpf(float(v))) for v in x]
    return [mpmath.power(mpmath.mpf(float(a)), mpmath.mpf(float(b))) for a, b in zip(x, y)]


def _rel_err(got, truth, single):
    if single:
        t = np.asarray(truth)
        ok = np.abs(t) > float(np.finfo(np.float32).tiny)
        return float(np.max(np.abs(np.asarray(got, np.longdouble)[ok] - t[ok]) / np.abs(t[ok])))
    import mpmath
    tiny = float(np.finfo(np.float64).tiny)
    return max([float(abs(mpmath.mpf(float(g)) - t) / abs(t)) for g, t in zip(got, truth) if abs(t) > tiny] or [0.0])


def probe(fn, x, y=None):
    from flexpart_amd import _lib
    lib = _lib.load()
    xin = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64)] + ([np.asarray(y, np.float64)] if y is not None else [])))
    out = np.empty(len(x))
    _lib.check(lib.fpx_math_probe(int(fn), xin.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(x)), "fpx_math_probe")
    return out


def device_bound(c, recs, kind):
    """The per-particle relative bound of THE RULE for every ohreaction of the case -> (list of [3][n] arrays, the measured
    worst relative errors of the device's exp and pow)."""
    single = kind == "r4"
    rt = oref.RT[kind]
    eps = float(np.finfo(rt).eps)
    temps = np.unique(np.concatenate([r["rec"]["temp"][r["rec"]["react"]] for r in recs]))
    grid_t = np.concatenate([temps, np.linspace(200.0, 288.0, 1500)]).astype(rt).astype(np.float64)
    u_pow = 0.0
    for k in (0, 2):
        nc = np.full(grid_t.size, float(rt(c["ohnconst"][k])))
        u_pow = max(u_pow, _rel_err(probe(43 if single else 42, grid_t, nc), _truth("pow", grid_t, nc, single), single))
    args = []
    for r in recs:
        rec = r["rec"]
        tl = float(abs(r["ltsample"]))
        for k in (0, 2):
            t = rec["temp"][rec["react"]].astype(rt)
            args.append((-rt(c["ohdconst"][k]) / t).astype(np.float64))
            x = rec["rates"][k][rec["react"]] * tl
            args.append(-x[~rec["zeroed"][k][rec["react"]]])                      # (a zeroed mass is compared bitwise, not by the bound)
    a = np.concatenate(args)
    a = np.concatenate([a, np.linspace(a.min(), a.max(), 1500)]).astype(rt).astype(np.float64)
    u_exp = _rel_err(probe(41 if single else 40, a), _truth("exp", a, None, single), single)
    d_pow, d_exp = 2.0 * u_pow + eps, 2.0 * u_exp + eps
    rho = d_pow + d_exp + 4.0 * eps
    bounds = [np.expm1(r["rec"]["rates"] * float(abs(r["ltsample"])) * rho) + d_exp + eps for r in recs]
    return bounds, u_exp, u_pow


@pytest.mark.gpu
@pytest.mark.parametrize("ld", syn.OH_DIRECTIONS)
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_ohreaction_against_the_reference(built, gold, restated, cb, hb, ld):
    """The whole sequence of the case (the slot quirk with memind = (2, 1) in the second ohreaction included) by THE RULE; the
    second ohreaction starts from the fixture's masses after the first."""
    kind = kind_of(hb)
    c, res, _ = restated[kind, ld]
    want = gold_calls(gold[kind], c)
    eng = make_engine(c, cb, hb)
    got = run_calls(eng, c, reset_to={4: want[1]["xmass1"]})
    recs = [r for r in res if r["kind"] == "react"]
    bounds, u_exp, u_pow = device_bound(c, recs, kind)
    eps = float(np.finfo(oref.RT[kind]).eps)
    live = np.asarray(c["itra1"]) != oref.DEAD
    before = [syn.oh_masses(c, kind).astype(np.float64), want[1]["xmass1"].astype(np.float64)]
    worst_bound = worst_seen = 0.0
    for (i, r, b, m0) in zip((1, 4), recs, bounds, before):
        g, w = got[i], want[i]["xmass1"].astype(np.float64)
        rec = r["rec"]
        assert np.array_equal(g[:, ~live], m0[:, ~live])                          # dead spaces: untouched
        assert np.array_equal(g[1], w[1]) and np.array_equal(g[1], m0[1])          # species 2 never reacts
        dark = live & ~rec["react"]
        assert dark.sum() > 100 and np.array_equal(g[:, dark], w[:, dark]) and np.array_equal(g[:, dark], m0[:, dark])
        zeroed = rec["zeroed"] & live[None, :]
        assert zeroed.any() and (g[zeroed] == 0).all() and (w[zeroed] == 0).all()
        rest = live[None, :] & rec["react"][None, :] & ~rec["zeroed"]
        rest[1] = False
        assert rest.sum() > 300
        err = np.abs(g - w)[rest] / w[rest]
        worst_bound, worst_seen = max(worst_bound, float(b[rest].max())), max(worst_seen, float(err.max()))
        bad = err > b[rest]
        assert not bad.any(), (i, int(bad.sum()), float((err / b[rest]).max()))
        # one index off by one would show: the next cell's temperature or OH changes the mass by far more than the bound
        assert eng.info("oh_skipped") == int((rec["outside"] & live).sum()) == 0
    print(f"[{kind} ld={ld}] device exp: {u_exp / eps:.3f} eps, pow: {u_pow / eps:.3f} eps (worst relative error over the case's arguments); "
          f"worst bound {worst_bound / eps:.1f} eps, worst observed {worst_seen / eps:.2f} eps")
    assert eng.ohreaction_time() > 0.0
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_storage_order_and_split_do_not_matter(built, cb, hb):
    """The same cloud after fpx_sort_particles, and uploaded as two halves into two handles one after the other: masses per
    particle number bitwise equal to the unsorted, single-handle run."""
    kind = kind_of(hb)
    c = syn.oh_case(1)
    calls = c["calls"][:2]
    eng = make_engine(c, cb, hb)
    plain = run_calls(eng, c, calls)[1]
    eng.close()
    eng = make_engine(c, cb, hb)
    eng.sort()
    sorted_ = run_calls(eng, c, calls)[1]
    eng.close()
    assert np.array_equal(plain, sorted_)
    n, half = int(c["npart"]), 419
    parts = []
    for sel in (slice(0, half), slice(half, n)):
        eng = make_engine(c, cb, hb, sel=sel)
        parts.append(run_calls(eng, c, calls)[1])
        eng.close()
    assert np.array_equal(plain, np.concatenate(parts, axis=1))
    assert (plain != syn.oh_masses(c, kind).astype(np.float64)).sum() > 300


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_checkpoint_across_the_hour(built, tmp_path, cb, hb):
    """A run continued from a checkpoint written between the first ohreaction and the advance at the hour equals the
    uninterrupted one bit for bit (xmass1, OH_hourly, memOHtime: the hourly fields cannot be recomputed from itime).  A handle
    without OH writes byte for byte what it wrote before the feature; a mismatch is refused both ways, nothing touched."""
    from flexpart_amd._lib import FpxError
    c = syn.oh_case(-1)
    eng = make_engine(c, cb, hb)
    whole = run_calls(eng, c)
    eng.close()
    a = make_engine(c, cb, hb)
    run_calls(a, c, c["calls"][:2])
    ck = str(tmp_path / "oh.ckpt")
    a.checkpoint_write(ck, itime=900)
    a.close()
    b = make_engine(c, cb, hb)
    b.checkpoint_read(ck)
    rest = run_calls(b, c, c["calls"][2:])
    for g, w in zip(rest, whole[2:]):
        if isinstance(g, tuple):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2]
        else:
            assert np.array_equal(g, w)
    # without OH: the file of a handle that never saw fpx_oh_init, twice, and bit 3 of header.reserved clear
    plain = make_engine(c, cb, hb, oh=False)
    f1, f2 = str(tmp_path / "p1.ckpt"), str(tmp_path / "p2.ckpt")
    plain.checkpoint_write(f1, itime=900)
    other = make_engine(c, cb, hb, oh=False)
    other.checkpoint_write(f2, itime=900)
    d1 = open(f1, "rb").read()
    assert d1 == open(f2, "rb").read()
    cells = int(np.prod(c["ohgrid"]))
    assert os.path.getsize(ck) == len(d1) + 16 + (2 + 2 * cells) * hb           # the OH section: count, presence, memOHtime, two fields
    before = b.download()["xmass1"]
    with pytest.raises(FpxError) as e:
        b.checkpoint_read(f1)                                                    # written without OH, read with
    assert e.value.code == ERR_STATE and "OH" in str(e.value)
    assert np.array_equal(b.download()["xmass1"], before)
    before = plain.download()["xmass1"]
    with pytest.raises(FpxError) as e:
        plain.checkpoint_read(ck)                                                # written with OH, read without
    assert e.value.code == ERR_STATE and "OH" in str(e.value)
    assert np.array_equal(plain.download()["xmass1"], before)
    for x in (b, plain, other):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_states_and_refusals(built, cb, hb):
    from flexpart_amd._lib import FpxError, FpxOhConfig
    c = syn.oh_case(1)

    def refused(fn, code, *words):
        with pytest.raises(FpxError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    eng = make_engine(c, cb, hb, oh=False, tt_slots=(2,))
    refused(lambda: eng.ohreaction(900, 900), ERR_STATE, "fpx_oh_init")
    refused(lambda: eng.gethourlyOH(0), ERR_STATE, "fpx_oh_init")
    refused(lambda: eng.oh_init(c, struct_bytes=C.sizeof(FpxOhConfig) + 8), ERR_ARG, "size mismatch")
    bad = dict(c)
    bad["lonOH"] = np.array(c["lonOH"])[[0, 1, 3, 2, 4, 5, 6, 7, 8]]
    refused(lambda: eng.oh_init(bad), ERR_UNSUPPORTED, "lonOH", "does not increase strictly")
    bad = dict(c)
    bad["altOH"] = np.array([500.0, 2000.0, 1000.0, 10000.0])
    refused(lambda: eng.oh_init(bad), ERR_UNSUPPORTED, "altOHtop")
    eng.oh_init(c)
    eng.set_windtime((0, 10800), (1, 2))
    refused(lambda: eng.ohreaction(900, 900), ERR_STATE, "fpx_gethourlyOH")
    eng.gethourlyOH(0)
    refused(lambda: eng.ohreaction(900, 900), ERR_STATE, "tt of time slot 1")       # n = 1 (ohreaction.f90:85-87), only slot 2 is there
    eng.ohreaction(9900, 900)                                                      # n = 2
    eng.close()
    big = dict(c)
    big["nest"] = (14, 6)                                                          # nxn > nx
    eng = make_engine(big, cb, hb, oh=False)
    refused(lambda: eng.oh_init(c), ERR_UNSUPPORTED, "nxn > nx")
    eng.close()


@pytest.mark.gpu
def test_a_handle_without_oh_launches_what_it_launched(built):
    """A step on a handle that was never given OH data and on one that was: the same kernels, the same launch count."""
    c = syn.oh_case(1)
    counts, masses = [], []
    for oh in (False, True):
        eng = make_engine(c, 8, 8, oh=oh, nest=False)
        eng.step()
        counts.append(eng.kernel_times()[1])
        masses.append(eng.download()["xmass1"])
        eng.close()
    assert counts[0] == counts[1] == 1
    assert np.array_equal(masses[0], masses[1])
