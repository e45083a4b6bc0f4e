"""The 256-entry exponential of the fp64 gas Langevin kernels (kExpTab256, m_exp_tab<256, 4>, m_exp_tab_nh<256, 4> in
fpx_device.hpp) and the LDS budget of the finer tables.

CPU: the committed table is 2**(j/256) correctly rounded, and an exact mirror of the device form -- every fma, product and
rint rounded once, as the hardware does, through rational arithmetic -- stays within one ulp (2**-52 relative: the rounding of
the table entry plus that of the final fma) of mpmath on 3500 points of -700 .. 0; the 32-entry form's figures on the same
points are printed next to it.  GPU: the device forms through fpx_math_probe (fn 32, 33) against the same truth, the form with
the factor -1/2 in its constants against the plain one bit for bit, the special values against the 32-entry pair (fn 9, 14),
and the engine: an fp64 gas CBL cloud at nz = 138 keeps three blocks per CU with the larger tables, in one launch and sliced.
"""
import ctypes as C
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from flexpart_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_HPP = os.path.join(ROOT, "flexpart_amd", "csrc", "fpx_device.hpp")
ONE_ULP = 2.0 ** -52

# (entries, degree) -> N/ln2, the two parts of ln2/N, log2 N: the constants of ExpTabConst in fpx_device.hpp
FORMS = {
    (32, 6): (46.16624130844683, 0.02166084938653512, 5.9631716539705866e-12, 5),
    (256, 4): (369.3299304675746, 0.00270760617331689, 7.453964567463233e-13, 8),
}
FACTORIALS = [1.0, 1.0, 0.5, 1.6666666666666666667e-01, 4.1666666666666666667e-02, 8.3333333333333333333e-03, 1.3888888888888888889e-03]


def header_array(name, n):
    text = open(DEVICE_HPP).read()
    body = text[text.index("%s[%d] = {" % (name, n)):]
    body = body[body.index("{") + 1:body.index("};")]
    vals = [float(t) for t in re.findall(r"[0-9]+\.[0-9]+(?:e[-+]?[0-9]+)?", body)]
    assert len(vals) == n, (name, len(vals))
    return vals


@functools.lru_cache(maxsize=None)
def tables():
    return {32: header_array("kExpTab", 32), 256: header_array("kExpTab256", 256)}


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # one rounding, to nearest even


def mirror(x, entries, degree, nh=False):
    """m_exp_tab<entries, degree>(x), or m_exp_tab_nh<entries, degree>(x) = exp(-x/2), operation by operation"""
    per_ln2, hi, lo, bits = FORMS[(entries, degree)]
    s = -0.5 if nh else 1.0                                      # the power of two the _nh form folds into its constants
    k = float(round(x * (s * per_ln2)))                          # v_rndne_f64: half to even, as Python's round
    r = fma(k, -hi / s, x)
    r = fma(k, -lo / s, r)
    ki = int(k)
    t = tables()[entries][ki & (entries - 1)]
    # (exp(r) - 1)/r to r**(degree - 1); the _nh form's coefficient of r**j carries s**(j + 1)
    c = [FACTORIALS[j + 1] * s ** (j + 1) for j in range(degree)]
    p = c[degree - 1]
    for j in range(degree - 2, -1, -1):
        p = fma(r, p, c[j])
    return float(np.ldexp(fma(t, r * p, t), ki >> bits))


@functools.lru_cache(maxsize=None)
def points():
    """about 3500 points of -700 .. 0 and mpmath's exp there (50 digits)"""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(14)
    x = np.concatenate([rng.uniform(-700.0, 0.0, 3000), rng.uniform(-40.0, 0.0, 300), rng.uniform(-1e-3, 0.0, 100),
                        -np.log(2.0) / 512 * np.arange(1, 97, 2.0), [0.0, -1e-300, -700.0]])
    assert 3400 < x.size < 3600 and x.min() >= -700.0 and x.max() <= 0.0
    return x, [mp.exp(mp.mpf(float(v))) for v in x]


def relative_errors(got, truth):
    import mpmath as mp
    return np.array([float(abs(mp.mpf(float(g)) - t) / t) for g, t in zip(got, truth)])


def figures(name, err):
    u = err / 2.0 ** -53
    print("[exp table] %-22s worst %.3f, 99.9 %% %.3f, median %.3f  (units of 2**-53, %d points)" % (
        name, u.max(), np.quantile(u, 0.999), np.median(u), u.size))
    return err.max()


def test_table_is_two_to_the_j_over_256_correctly_rounded():
    import mpmath as mp
    mp.mp.dps = 50
    t256, t32 = tables()[256], tables()[32]
    want = [float(mp.power(2, mp.mpf(j) / 256)) for j in range(256)]
    assert t256 == want
    assert t256[::8] == t32                                      # the 32-entry table is every eighth entry


def test_mirror_of_the_256_entry_form_is_within_an_ulp():
    x, truth = points()
    worst = {}
    for form in ((32, 6), (256, 4)):
        got = [mirror(float(v), *form) for v in x]
        worst[form] = figures("%d entries, degree %d:" % form, relative_errors(got, truth))
    assert worst[(256, 4)] <= ONE_ULP


def test_mirror_of_the_prescaled_form_has_the_same_bits():
    u = np.concatenate([np.random.default_rng(5).uniform(0.0, 1400.0, 400), [0.0, 1e-300, 36.0]])
    for form in ((32, 6), (256, 4)):
        a = np.array([mirror(float(v), *form, nh=True) for v in u])
        b = np.array([mirror(-(0.5 * float(v)), *form) for v in u])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), form


def probe(fn, x):
    from flexpart_amd import _lib
    lib = _lib.load()
    arg = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full(len(arg), -7.0)
    assert lib.fpx_math_probe(fn, arg.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(arg)) == 0
    return y


@pytest.mark.gpu
def test_device_form_is_within_an_ulp(built):
    x, truth = points()
    worst = {}
    for name, fn in (("32 entries (fn 9):", 9), ("256 entries (fn 32):", 32)):
        worst[fn] = figures(name, relative_errors(probe(fn, x), truth))
    assert worst[32] <= ONE_ULP
    # the device runs what the mirror states
    got = probe(32, x)
    want = np.array([mirror(float(v), 256, 4) for v in x])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.gpu
def test_prescaled_device_form_has_the_same_bits(built):
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.uniform(0.0, 80.0, 3000), rng.uniform(0.0, 1e-3, 200), rng.uniform(0.0, 1400.0, 300), [0.0, 1e-300, 36.0, 1e4]])
    a = probe(33, u)
    b = probe(32, -(0.5 * u))
    assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert a[-4] == 1.0 and a[-3] == 1.0 and a[-1] == 0.0


@pytest.mark.gpu
def test_special_values_behave_as_in_the_32_entry_form(built):
    # an infinite argument gives NaN in both forms (the range reduction subtracts infinities), as NaN does: the class is
    # compared there, not sign and payload; everywhere else the value
    special = np.array([0.0, -0.0, 1e-300, -1e-300, 1e4, -1e4, np.inf, -np.inf, np.nan])
    for fine, coarse in ((32, 9), (33, 14)):
        a, b = probe(fine, special), probe(coarse, special)
        nan = np.isnan(b)
        assert np.array_equal(nan, ~np.isfinite(special)), coarse
        assert np.array_equal(np.isnan(a), nan), fine
        assert np.array_equal(a[~nan], b[~nan]), (fine, a, b)
    assert np.array_equal(probe(32, special)[:6], [1.0, 1.0, 1.0, 1.0, np.inf, 0.0])
    assert np.array_equal(probe(33, special)[:6], [1.0, 1.0, 1.0, 1.0, 0.0, np.inf])


@pytest.mark.gpu
@pytest.mark.parametrize("slice_passes", [-1, 3])
def test_gas_kernel_keeps_three_blocks_per_cu(built, slice_passes):
    """One launch (19 stash slots) and time slices (the twin with 20): 50896 B and 52944 B of LDS per block at nz = 138."""
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = syn.small(n=4096, nx=40, ny=24, nz=138, nsteps=1, ctl=5.0, ifine=4, cblflag=1)
    eng = Engine(sc, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_PHILOX, seed=3, pbl_slice_passes=slice_passes)
    eng.step()
    per_cu, launches = eng.info("pbl_blocks_per_cu"), eng.info("pbl_launches_per_step")
    out = eng.download()
    eng.close()
    assert (launches == 1) == (slice_passes < 0), launches
    assert per_cu == 3, per_cu
    for k in ("xtra1", "ytra1", "ztra1", "uzp"):
        assert np.all(np.isfinite(out[k])), k
