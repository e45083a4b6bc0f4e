"""One cubic refinement step behind the seeds of the fp64 root and reciprocal helpers (fpx_device.hpp, DESIGN.md "Round 8").

CPU: tools/newton_tail_model.py, both forms of every helper in exact arithmetic from seeds perturbed by 2^-23 (v_rcp_f64,
v_rsq_f64) and 2^-19 (the f32 seeds): every cubic form within the 2 ulp the header of fpx_device.hpp states.

GPU, through fpx_math_probe:
  - each changed helper against mpmath on about 2e4 points (helper_points): 2 ulp for the hardware-seeded ones, for the
    f32-seeded ones the bounds tests/test_gpu_parity.py::test_device_math_helpers_against_libm has for them (4 ulp relative for
    m_rcbrt, 3e-15 relative for m_pow08, 4 ulp * (1 + |ln x|) for the two results of m_cuberoot_parts), and for every helper a worst
    error at most 0.5 ulp above the worst error of the form with two quadratic steps (probe numbers 19 .. 27, 31) on the same points;
  - the same class of result as the two-step form for 0, -0, infinities, NaN, negative and subnormal arguments;
  - the raw seeds (probe numbers 15 .. 18) against the error a cubic step can take: C * e0^3 <= 2^-56 with C the third-order
    coefficient of the series in the residual (1, 5/16, 1/2, 14/81, 0.088), over the whole range of each seed.  The residual of
    a root of order k is k times the seed's error, so the bound that decides is k^3 times tighter in e0
    (THIRD_ORDER_IN_SEED_ERROR of the model: 1, 5/2, 5/2, 14/3, 11); that one is asserted where the helpers take the cubic step (the f32 seeds: CUBIC_WINDOW).
  - the stable and neutral regimes of hanna() / hanna_short() and the free troposphere against the CPU oracle, at the fp64
    tolerances of tests/test_gpu_parity.py with no diverged particle.
"""
import ctypes as C
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

from flexpart_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
TOL_POS, TOL_VEL = 1e-9, 1e-7
N, NSTEPS = 6000, 3


@functools.lru_cache(maxsize=None)
def model():
    spec = importlib.util.spec_from_file_location("newton_tail_model", os.path.join(ROOT, "tools", "newton_tail_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the model
# ---------------------------------------------------------------------------------------------------------------------------
def test_model_cubic_forms_within_two_ulp():
    res = model().run({"rcp": 2.0 ** -23, "rsq": 2.0 ** -23, "cbrt": 2.0 ** -19, "fifth": 2.0 ** -19}, points=2000)
    print({k: {f: round(v, 3) for f, v in w.items()} for k, w in res.items()})
    for name in ("rcp", "rsqrt", "sqrt", "sqrt_rsqrt.s", "sqrt_rsqrt.rs", "rcbrt", "x^-1/5"):
        assert res[name]["c1"] <= 2.0, (name, res[name])
    # m_pow08 = x * x^(-1/5) carries one more rounding than the root; its bound is the one its parity test has (3e-15 relative,
    # which is at least 6.7 ulp of the result)
    assert res["pow08"]["c1"] <= 3e-15 / (2.0 * ULP), res["pow08"]


def test_cubic_coefficients_are_the_series():
    """(1 - e)^(-1/k) = 1 + e/k + (k+1)/(2 k^2) e^2 + (k+1)(2k+1)/(6 k^3) e^3: the second-order coefficients the forms use and
    the third-order ones the seed bounds use"""
    from fractions import Fraction as F
    for k, c2, c3 in ((1, 1.0, 1.0), (2, 0.375, 5.0 / 16.0), (3, 2.0 / 9.0, 14.0 / 81.0), (5, 0.12, 0.088)):
        assert float(F(k + 1, 2 * k * k)) == c2 and abs(float(F((k + 1) * (2 * k + 1), 6 * k ** 3)) - c3) < 1e-15
    m = model()
    assert m.THIRD_ORDER == {"rcp": 1.0, "rsq": 5.0 / 16.0, "sqrt": 0.5, "cbrt": 14.0 / 81.0, "fifth": 0.088}
    for use, k in (("rcp", 1), ("rsq", 2), ("cbrt", 3), ("fifth", 5)):       # residual = k * seed error
        assert abs(m.THIRD_ORDER_IN_SEED_ERROR[use] - m.THIRD_ORDER[use] * k ** 3) < 1e-12
    assert m.THIRD_ORDER_IN_SEED_ERROR["sqrt"] == m.THIRD_ORDER_IN_SEED_ERROR["rsq"]       # (1 - 2r)^(-1/2) = 1 + r + 3/2 r^2 + 5/2 r^3, r = e0
    assert abs(math.log2(m.eps0_bound(1.0)) + 56.0 / 3.0) < 1e-12


def test_tolerances_are_those_of_the_parity_tests():
    import test_gpu_parity as tp
    for fn in (tp.test_fp64_matches_oracle, tp.test_fp64_matches_oracle_golden_scenarios):
        assert {TOL_POS, TOL_VEL} <= set(fn.__code__.co_consts), fn.__name__
    consts = tp.test_device_math_helpers_against_libm.__code__.co_consts
    assert 3e-15 in consts and (4 * ULP in consts or 4 in consts)      # m_pow08's bound and the "4 ulp" of ulp4


# ---------------------------------------------------------------------------------------------------------------------------
# points and references
# ---------------------------------------------------------------------------------------------------------------------------
EXPONENTS = (-120, -30, -1, 0, 1, 30, 120)


@functools.lru_cache(maxsize=None)
def mantissa_points():
    """mantissas 1, 1 + ulp, 2 - ulp (at the exponent below: 1 - ulp/2), sqrt(2) -+ ulp and 2800 random ones, at EXPONENTS"""
    rng = np.random.default_rng(8)
    r2 = math.sqrt(2.0)
    m = np.concatenate([[1.0, 1.0 + ULP, 2.0 - ULP, 1.0 - ULP / 2, np.nextafter(r2, 0.0), r2, np.nextafter(r2, 2.0)], 1.0 + rng.random(2800)])
    return np.concatenate([np.ldexp(m, e) for e in EXPONENTS])


@functools.lru_cache(maxsize=None)
def helper_points(kind):
    """kind: "pos" (rsqrt, sqrt_rsqrt), "sqrt" (0, the smallest normal, perfect squares added), "signed" (rcp, divf: both signs),
    "f32" (the f32-seeded roots: powers of two of the seed range only, its two ends, 1e-37, 1e-3, 1)"""
    base = mantissa_points()
    if kind == "f32":
        return np.concatenate([base, np.ldexp(1.0, np.arange(-122, 122)), [2.0 ** -122, np.nextafter(2.0 ** 122, 0.0), 1e-37, 1e-3, 1.0]])
    pos = np.concatenate([base, np.ldexp(1.0, np.arange(-1000, 1001, 4)), np.ldexp(1.0, np.arange(-121, 122))])
    if kind == "pos":
        return pos
    if kind == "sqrt":
        k = np.arange(1.0, 400.0)
        return np.concatenate([pos, [0.0, np.finfo(np.float64).tiny], k * k, (k * 65537.0) ** 2])
    assert kind == "signed"
    return np.concatenate([pos, -pos])


def _mp():
    import mpmath as mp
    mp.mp.prec = 200
    return mp


TRUE = {
    "rcp": lambda mp, x: 1 / x,
    "div3": lambda mp, x: 3 / x,
    "sqrt": lambda mp, x: mp.sqrt(x),
    "rsqrt": lambda mp, x: 1 / mp.sqrt(x) if x else mp.inf,
    "rcbrt": lambda mp, x: 1 / mp.root(x, 3),
    "pow08": lambda mp, x: mp.power(x, mp.mpf(0.8)),
    "c": lambda mp, x: mp.power(x, mp.mpf(0.333333333)),
    "ic2": lambda mp, x: mp.power(x, -2 * mp.mpf(0.333333333)),
    "rfifth": lambda mp, x: 1 / mp.root(x, 5),
}


@functools.lru_cache(maxsize=None)
def reference(what, kind):
    """mpmath's value of `what` at helper_points(kind) as an unevaluated sum hi + lo of two doubles (relative 2^-105)"""
    mp = _mp()
    x = helper_points(kind)
    hi, lo = np.empty_like(x), np.empty_like(x)
    for i, v in enumerate(x):
        t = TRUE[what](mp, mp.mpf(float(v)))
        hi[i] = float(t)
        lo[i] = float(t - mp.mpf(float(hi[i])))
    hi.setflags(write=False)
    lo.setflags(write=False)
    return hi, lo


def ulp_errors(got, ref):
    """|got - ref| in units of the last place of ref"""
    hi, lo = ref
    with np.errstate(invalid="ignore", divide="ignore"):
        ulp = np.ldexp(1.0, np.frexp(hi)[1] - 53)
        err = np.abs((got - hi) - lo) / ulp
    return np.where(hi == 0.0, np.where(got == 0.0, 0.0, np.inf), err)


def rel_errors(got, ref):
    hi, lo = ref
    return np.abs((got - hi) - lo) / np.abs(hi)


def probe(fn, x):
    from flexpart_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    assert lib.fpx_math_probe(fn, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size) == 0
    return y


# helper -> (probe number as the kernels call it, probe number of the form with two quadratic steps, points, reference)
HW_HELPERS = {
    "m_rcp": (3, 19, "signed", "rcp"),
    "m_divf": (30, 31, "signed", "div3"),
    "m_rsqrt": (4, 20, "pos", "rsqrt"),
    "m_sqrtp": (2, 21, "sqrt", "sqrt"),
    "m_sqrt_rsqrt.s": (28, 22, "pos", "sqrt"),
    "m_sqrt_rsqrt.rs": (29, 23, "pos", "rsqrt"),
}
F32_HELPERS = {
    "m_rcbrt": (11, 24, "rcbrt"),
    "m_pow08": (8, 25, "pow08"),
    "m_cuberoot_parts.c": (5, 26, "c"),
    "m_cuberoot_parts.ic2": (6, 27, "ic2"),
}


def test_point_sets_are_what_the_docstring_says():
    for kind in ("pos", "sqrt", "signed", "f32"):
        x = helper_points(kind)
        assert 1.9e4 <= x.size <= 4.5e4, (kind, x.size)
    f = helper_points("f32")
    assert 2.0 ** -122 in f and f.max() == np.nextafter(2.0 ** 122, 0.0) and f.min() == 1e-37   # 1e-37: the floor zeta_powers() gives m_rcbrt, under the range
    s = helper_points("sqrt")
    assert (s == 0.0).sum() == 1 and np.finfo(np.float64).tiny in s and 49.0 in s
    assert (helper_points("signed") < 0).sum() * 2 == helper_points("signed").size


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HW_HELPERS))
def test_hardware_seeded_helper_against_mpmath(built, name):
    fn, fn_q2, kind, what = HW_HELPERS[name]
    x, ref = helper_points(kind), reference(what, kind)
    e_now, e_q2 = ulp_errors(probe(fn, x), ref), ulp_errors(probe(fn_q2, x), ref)
    print(f"{name}: worst error {e_now.max():.3f} ulp at {x[e_now.argmax()]!r}; two quadratic steps {e_q2.max():.3f} ulp at {x[e_q2.argmax()]!r}; {x.size} points")
    assert e_now.max() <= 2.0
    assert e_now.max() <= e_q2.max() + 0.5
    if name == "m_sqrtp":
        z = probe(fn, np.array([0.0]))
        assert z[0] == 0.0 and not np.signbit(z[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(F32_HELPERS))
def test_f32_seeded_helper_against_mpmath(built, name):
    fn, fn_q2, what = F32_HELPERS[name]
    x, ref = helper_points("f32"), reference(what, "f32")
    got, got_q2 = probe(fn, x), probe(fn_q2, x)
    e_now, e_q2 = ulp_errors(got, ref), ulp_errors(got_q2, ref)
    rel = rel_errors(got, ref)
    print(f"{name}: worst error {e_now.max():.3f} ulp ({rel.max():.3e} relative) at {x[e_now.argmax()]!r}; two quadratic steps {e_q2.max():.3f} ulp; {x.size} points")
    w = (x >= CUBIC_WINDOW[0]) & (x < CUBIC_WINDOW[1])          # where the cubic step is taken: outside it the two forms are one
    print(f"{name} where the cubic step is taken: worst error {e_now[w].max():.3f} ulp; two quadratic steps {e_q2[w].max():.3f} ulp; {w.sum()} points")
    assert e_now[w].max() <= e_q2[w].max() + 0.5
    if name == "m_rcbrt":
        assert rel.max() < 4 * ULP
    elif name == "m_pow08":
        assert rel.max() < 3e-15
    else:
        assert np.max(rel / (4 * ULP * (1.0 + np.abs(np.log(x))))) < 1.0
    assert e_now.max() <= e_q2.max() + 0.5


def result_class(y):
    return np.where(np.isnan(y), 0, np.where(np.isinf(y), 1, np.where(y == 0.0, 2, 3))) * np.where(np.isnan(y), 1, np.where(np.signbit(y), -1, 1))


@pytest.mark.gpu
def test_special_arguments_keep_their_class(built):
    """0, -0, +-inf, NaN, negative numbers and subnormals: NaN, an infinity, a zero or a finite number of the same sign from the
    cubic form wherever the two-step form gives one.  What that is per helper is written at the helper (fpx_device.hpp)."""
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-300, -1e300, 5e-324, 1e-310, -1e-310, 1e-300, 1e300, 1.7e308])
    for name, (fn, fn_q2, *_) in sorted({**HW_HELPERS, **{k: v[:2] for k, v in F32_HELPERS.items()}}.items()):
        if name == "m_rcbrt":
            continue            # no argument outside the f32 seed range reaches it (zeta_powers, m_pow13 screen them)
        a, b = probe(fn, sp), probe(fn_q2, sp)
        print(name, a, b)
        assert np.array_equal(result_class(a), result_class(b)), (name, a, b)


SEEDS = {
    "rcp": (15, "signed", "rcp", ("rcp",)),
    "rsq": (16, "pos", "rsqrt", ("rsq", "sqrt")),
    "cbrt": (17, "f32", "rcbrt", ("cbrt",)),
    "fifth": (18, "f32", "rfifth", ("fifth",)),
}


def seed_error(seed):
    fn, kind, what, _ = SEEDS[seed]
    x = helper_points(kind)
    rel = rel_errors(probe(fn, x), reference(what, kind))
    return x, rel


# the f32 seeds lose accuracy with |log2 x|: the helpers take the cubic step for 2^-48 <= x < 2^64 only (m_in_cubic_range)
CUBIC_WINDOW = (2.0 ** -48, 2.0 ** 64)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sorted(SEEDS))
def test_seed_is_good_enough_for_a_cubic_step(built, seed):
    m = model()
    x, rel = seed_error(seed)
    e0 = float(rel.max())
    used = (x >= CUBIC_WINDOW[0]) & (x < CUBIC_WINDOW[1]) if SEEDS[seed][1] == "f32" else np.ones(x.size, bool)
    assert 0.25 * x.size < used.sum()
    e0_used = float(rel[used].max())
    print(f"seed {seed}: e0 = {e0:.3e} = 2^{math.log2(e0):.2f} at {x[rel.argmax()]!r} ({x.size} points); where the cubic step is taken 2^{math.log2(e0_used):.2f} ({used.sum()} points)")
    for use in SEEDS[seed][3]:
        c = m.THIRD_ORDER[use]
        stated = m.eps0_bound(c)                                   # C * e0^3 <= 2^-56
        residual = m.eps0_bound(m.THIRD_ORDER_IN_SEED_ERROR[use])      # the same with the residual written in e0
        print(f"  {use}: C = {c:.4g}, bound 2^{math.log2(stated):.2f}, on the residual 2^{math.log2(residual):.2f}")
        assert e0 <= stated, (use, e0, stated)
        assert e0_used <= residual, (use, e0_used, residual)


# ---------------------------------------------------------------------------------------------------------------------------
# the regimes tests/test_cbl_folds.py does not reach, against the CPU oracle
# ---------------------------------------------------------------------------------------------------------------------------
RECIPES = ("hanna", "above_pbl_only")


@functools.lru_cache(maxsize=None)
def scenario(recipe, nz):
    from test_oracle_cpu import CASES
    sc = syn.small(n=N, nx=48, ny=32, nz=nz, nsteps=NSTEPS, ldirect=1, **CASES[recipe])
    assert int(sc["cblflag"]) == 0 and len(sc["height"]) == nz
    return sc


def regime_fractions(sc):
    """share of the cloud that starts below the mixing height of its cell in a stable (1/L > 0 and h/L >= 1), a neutral
    (h/|L| < 1) and an unstable column, at the first wind-field time"""
    h, oli = np.asarray(sc["hmix"])[0], np.asarray(sc["oli"])[0]
    ix = np.asarray(sc["xtra1"]).astype(int) % h.shape[1]
    jy = np.minimum(np.asarray(sc["ytra1"]).astype(int), h.shape[0] - 1)
    inside = np.asarray(sc["ztra1"]) < h[jy, ix]
    hol = (h * oli)[jy, ix]
    return (inside & (hol >= 1.0)).mean(), (inside & (np.abs(hol) < 1.0)).mean(), (inside & (hol <= -1.0)).mean()


def test_the_recipes_reach_the_regimes():
    for nz in (138, 3):
        stable, neutral, unstable = regime_fractions(scenario("hanna", nz))
        assert stable > 0.05 and neutral > 0.02 and unstable > 0.05, (nz, stable, neutral, unstable)
        assert sum(regime_fractions(scenario("above_pbl_only", nz))) < 0.02


def _oracle_run(sc):
    from oracle.oracle import Oracle
    orc = Oracle(sc, "r8")
    orc.lib.orc_set_parallel_semantics(orc.h, 1)
    return orc.run(NSTEPS)


@pytest.mark.parametrize("recipe,nz", [(r, nz) for r in RECIPES for nz in (138, 3)])
def test_the_seeds_are_not_at_a_truncation_edge(recipe, nz):
    """The oracle against itself: the same cloud with every height moved to the next double.  A particle whose sub-step count
    int(...) sits at an integer would take another number of sub-steps and count as diverged; with this recipe's seed none does, so
    max_diverged = 0 asks of the engine only what rounding leaves open."""
    from oracle import oracle as orc_mod
    from test_gpu_parity import assert_close
    orc_mod.build()
    sc = scenario(recipe, nz)
    nudged = dict(sc, ztra1=np.nextafter(np.asarray(sc["ztra1"]), np.inf))
    for a, b in zip(_oracle_run(sc), _oracle_run(nudged)):
        assert assert_close(a, b, TOL_POS, TOL_VEL, max_diverged=0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,nz", [(r, nz) for r in RECIPES for nz in (138, 3)])
def test_other_regimes_against_the_oracle(built, recipe, nz):
    from test_gpu_parity import assert_close, run_pair
    sc = scenario(recipe, nz)
    got, want = run_pair(sc, "r8")
    assert len(got) == NSTEPS
    for g, w in zip(got, want):
        assert assert_close(g, w, TOL_POS, TOL_VEL, max_diverged=0) == 0
    assert (got[-1]["ztra1"] != np.asarray(sc["ztra1"])).mean() > 0.5
