"""The piecewise table of exp(x*x)*erfc(x) behind the error-function pair of cbl() (fpx_erfcx_tab.hpp, m_erf_tab2).

CPU: the committed header is what tools/fit_erfcx_table.py prints, and its coefficients, evaluated with numpy in double the
way the kernel does, give erf within 5e-16 absolute -- the bound m_erf_e documents -- on a grid of 0 .. 6.5 with every interval
edge and an ulp either side of it.  GPU: the table form and the polynomial form on the same (x, E) pairs through
fpx_math_probe (fn 13 and 12), each within that bound of mpmath's erf, at the edges named below, and the same class of result
for NaN and the infinities; and the exponential with the factor -1/2 in its constants (fn 14) has the bits of the plain one.
"""
import ctypes as C
import functools
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "flexpart_amd", "csrc", "fpx_erfcx_tab.hpp")
BOUND = 5e-16


@functools.lru_cache(maxsize=None)
def fit_script():
    spec = importlib.util.spec_from_file_location("fit_erfcx_table", os.path.join(ROOT, "tools", "fit_erfcx_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def header_table():
    """-> (rows [intervals][row], intervals per unit, degree, xmax) as the committed header states them"""
    text = open(HEADER).read()
    ints = {k: int(v) for k, v in re.findall(r"(kErfcx(?:Intervals|Degree|Row)) = (\d+)", text)}
    per_unit = float(re.search(r"kErfcxPerUnit = ([0-9.]+)", text).group(1))
    xmax = float(re.search(r"kErfcxMax = ([0-9.]+)", text).group(1))
    body = text[text.index("kErfcxTab["):]
    body = body[body.index("{") + 1:body.index("};")]
    vals = [float.fromhex(t) if "x" in t else float(t) for t in re.findall(r"-?0x[0-9a-f.]+p[-+]?\d+|-?\d+\.\d+", body)]
    rows = np.array(vals).reshape(ints["kErfcxIntervals"], ints["kErfcxRow"])
    assert ints["kErfcxRow"] % 2 == 0 and ints["kErfcxRow"] >= ints["kErfcxDegree"] + 2
    return rows, per_unit, ints["kErfcxDegree"], xmax


def edges_and_neighbours():
    rows, per_unit, degree, xmax = header_table()
    e = np.arange(0, len(rows) + 1) / per_unit
    e = e[e <= xmax]
    return np.unique(np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e[1:], -np.inf), [xmax, np.nextafter(xmax, 0.0)]]))


@functools.lru_cache(maxsize=None)
def mp_erf_and_gauss(xs):
    """mpmath at 40 digits: erf(x) as mpf, and exp(-x*x) rounded to double, for a tuple of finite doubles"""
    import mpmath as mp
    mp.mp.dps = 40
    erf = [mp.erf(mp.mpf(x)) for x in xs]
    E = np.array([float(mp.exp(-mp.mpf(x) * mp.mpf(x))) for x in xs])
    return erf, E


def worst_error(got, erf):
    import mpmath as mp
    return max(float(abs(mp.mpf(float(g)) - e)) for g, e in zip(got, erf))


def test_header_is_what_the_script_prints():
    fs = fit_script()
    best, report = fs.choose()
    assert fs.header(best) == open(HEADER).read()
    # the choice: the smallest candidate within the bound
    assert best[3] <= BOUND and all(r[0] >= best[0] for r in report if r[3] <= BOUND)


def test_table_reproduces_erf_in_double():
    rows, per_unit, degree, xmax = header_table()
    assert xmax == 6.5 and len(rows) == int(np.ceil(xmax * per_unit))
    assert np.array_equal(rows[:, 0], (np.arange(len(rows)) + 0.5) / per_unit)        # a row starts with its centre
    x = np.unique(np.concatenate([edges_and_neighbours(), np.linspace(0.0, xmax, 3001)]))
    erf, E = mp_erf_and_gauss(tuple(x))
    p = fit_script().eval_table(rows.tolist(), per_unit, degree, x)
    worst = worst_error(1.0 - E * p, erf)
    print("[erfcx table] worst |1 - E*p - erf| on %d points: %.3g" % (x.size, worst))
    assert worst <= BOUND


def probe(fn, x, E=None):
    from flexpart_amd import _lib
    lib = _lib.load()
    arg = np.ascontiguousarray(x if E is None else np.concatenate([x, E]), dtype=np.float64)
    y = np.full(len(x), -7.0)
    assert lib.fpx_math_probe(fn, arg.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), len(x)) == 0
    return y


@pytest.mark.gpu
def test_table_form_and_polynomial_form_on_the_device(built):
    rows, per_unit, degree, xmax = header_table()
    pos = np.unique(np.concatenate([edges_and_neighbours(), [1e-300, 6.5, 7.0], np.random.default_rng(11).uniform(0.0, 7.0, 1500)]))
    x = np.concatenate([[0.0, -0.0], pos[pos > 0], -pos[pos > 0]])
    assert 2000 < x.size < 5000
    erf, E = mp_erf_and_gauss(tuple(x))
    special = np.array([np.inf, -np.inf, np.nan])
    with np.errstate(invalid="ignore"):
        Es = np.exp(-special * special)
    xa, Ea = np.concatenate([x, special]), np.concatenate([E, Es])
    out = {}
    for name, fn in (("polynomial", 12), ("table", 13)):
        y = probe(fn, xa, Ea)
        out[name] = y
        worst = worst_error(y[:x.size], erf)
        print("[erf pair] %s form: worst |erf - mpmath| on %d points: %.3g" % (name, x.size, worst))
        assert worst <= BOUND, name
        assert y[x.size] == 1.0 and y[x.size + 1] == -1.0 and np.isnan(y[x.size + 2]), name
        # x = +-0: +-0 or an ulp of 1
        assert np.all(np.abs(y[:2]) <= 2.0 ** -52), name
    assert np.array_equal(np.isnan(out["table"]), np.isnan(out["polynomial"]))
    assert np.array_equal(np.isinf(out["table"]), np.isinf(out["polynomial"]))
    assert np.array_equal(out["table"][x.size:x.size + 2], out["polynomial"][x.size:x.size + 2])
    assert np.abs(out["table"][:x.size] - out["polynomial"][:x.size]).max() <= 2 * BOUND


@pytest.mark.gpu
def test_prescaled_exponential_has_the_same_bits(built):
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.uniform(0.0, 80.0, 3000), rng.uniform(0.0, 1e-3, 200), rng.uniform(0.0, 1500.0, 200), [0.0, 1e-300, 36.0, 1e4, np.inf, np.nan]])
    a = probe(14, u)
    b = probe(9, -(0.5 * u))
    # same bits wherever the result is a number; an infinite argument gives NaN in both forms (the range reduction subtracts
    # infinities), as NaN does: the class is compared there, not sign and payload
    nan = np.isnan(b)
    assert np.array_equal(nan, ~np.isfinite(u)) and np.array_equal(np.isnan(a), nan)
    assert np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
    assert u[-6] == 0.0 and a[-6] == 1.0 and u[-3] == 1e4 and a[-3] == 0.0
