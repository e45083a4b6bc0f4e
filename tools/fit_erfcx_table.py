#!/usr/bin/env python3
"""Fit the piecewise polynomial table of g(x) = exp(x*x)*erfc(x) that the Langevin kernel's error-function pair reads
(flexpart_amd/csrc/fpx_erfcx_tab.hpp, m_erf_tab2 in fpx_device.hpp).

    erf(x) = sign(x) * (1 - E*g(|x|)),  E = exp(-x*x) known to the caller

g is fitted on uniform intervals of x itself over 0 .. 6.5 (beyond 6.5 E < 5e-19 and the clamp is invisible): per interval a
polynomial in d = x - centre through the Chebyshev nodes of the interval, in 40-digit arithmetic, rounded to double.  A row of
the table is [centre, c_n, c_(n-1), .., c_0], padded with zeros to a multiple of 16 bytes so that rows stay aligned for
128-bit LDS loads (the kernel reads 64 bits at a time at present: it has no registers for wider reads in flight).

The width of an interval is set by the LDS budget of the kernel's block, the degree by the bound.  The fp64 gas instances have
about 10 KB of static LDS to spend at three blocks per CU (see kLdsTabDoubles in fpx_device.hpp): 104 intervals of width 1/16
fit (8320 B at degree 7), 208 of width 1/32 do not (13312 B at degree 6), and every halving of the width takes one to two
steps off the Horner chain that each sub-step of the kernel runs twice (width 1/4: degree 10, 2496 B; 1/8: degree 9, 4992 B).
So the script tries the degrees around the bound at width 1/16, reports for each the worst |1 - E*p(x) - erf(x)| of the
double-precision Horner evaluation (E = exp(-x*x) rounded to double, as the caller has it) over a grid that contains every
interval edge and an ulp either side of it, and takes the smallest table (in padded bytes) whose worst error is at or below
5e-16 -- the bound m_erf_e documents.

    python tools/fit_erfcx_table.py            # prints the header to stdout
    python tools/fit_erfcx_table.py --report   # prints the error report of every candidate instead
"""
from __future__ import annotations

import sys

import mpmath as mp
import numpy as np

mp.mp.dps = 40

XMAX = 6.5
BOUND = 5e-16
CANDIDATES = [(16, 6), (16, 7), (16, 8)]   # (intervals per unit of x, degree): the width-1/16 family


def g(x):
    return mp.exp(x * x) * mp.erfc(x)


def n_intervals(per_unit):
    return int(np.ceil(XMAX * per_unit))


def row_doubles(degree):
    n = degree + 2                      # centre + degree+1 coefficients
    return n + (n & 1)                  # padded to a multiple of 16 bytes


def fit(per_unit, degree):
    """rows[i] = [centre, c_degree, .., c_0, (0)] as Python floats"""
    half = mp.mpf(1) / (2 * per_unit)
    rows = []
    for i in range(n_intervals(per_unit)):
        centre = (mp.mpf(i) + mp.mpf(1) / 2) / per_unit
        n = degree + 1
        u = [mp.cos(mp.pi * (2 * k + 1) / (2 * n)) for k in range(n)]     # Chebyshev nodes on [-1, 1]
        A = mp.matrix(n, n)
        b = mp.matrix(n, 1)
        for r in range(n):
            for c in range(n):
                A[r, c] = u[r] ** c
            b[r] = g(centre + half * u[r])
        a = mp.lu_solve(A, b)                                             # polynomial in u = d/half
        coef = [float(a[k] / half ** k) for k in range(n)]                # ... in d (half is a power of two: exact)
        row = [float(centre)] + coef[::-1]
        row += [0.0] * (row_doubles(degree) - len(row))
        rows.append(row)
    return rows


def eval_table(rows, per_unit, degree, x):
    """1 - E*p as the kernel forms it (numpy, double), for x >= 0"""
    tab = np.asarray(rows)
    c = np.minimum(x, XMAX)
    i = np.minimum((c * float(per_unit)).astype(np.int64), len(rows) - 1)
    d = c - tab[i, 0]
    p = tab[i, 1].copy()
    for k in range(2, degree + 2):
        p = p * d + tab[i, k]
    return p


def grid(per_unit, dense=4000):
    edges = np.arange(0, n_intervals(per_unit) + 1) / float(per_unit)
    edges = edges[edges <= XMAX]
    pts = [edges, np.nextafter(edges, np.inf), np.nextafter(edges[1:], -np.inf), np.array([XMAX, np.nextafter(XMAX, 0.0)]),
           np.linspace(0.0, XMAX, dense), np.random.default_rng(7).uniform(0.0, XMAX, dense)]
    return np.unique(np.concatenate(pts))


def worst_error(rows, per_unit, degree):
    x = grid(per_unit)
    p = eval_table(rows, per_unit, degree, x)
    worst = 0.0
    for xi, pi in zip(x, p):
        xm = mp.mpf(float(xi))
        E = float(mp.exp(-xm * xm))                  # the caller's exp(-x*x), correctly rounded
        err = abs(mp.mpf(1.0 - E * float(pi)) - mp.erf(xm))
        worst = max(worst, float(err))
    return worst


def choose():
    report = []
    for per_unit, degree in CANDIDATES:
        rows = fit(per_unit, degree)
        size = len(rows) * row_doubles(degree) * 8
        report.append((size, per_unit, degree, worst_error(rows, per_unit, degree), rows))
    ok = [r for r in report if r[3] <= BOUND]
    if not ok:
        raise SystemExit("no candidate meets the bound")
    return min(ok, key=lambda r: r[0]), report


def header(best):
    size, per_unit, degree, worst, rows = best
    out = []
    out.append("// Generated by tools/fit_erfcx_table.py -- do not edit; change the script and run it again.")
    out.append("// g(x) = exp(x*x)*erfc(x) on 0 .. 6.5 as %d polynomials of degree %d in d = x - centre, one per interval of width 1/%d." % (len(rows), degree, per_unit))
    out.append("// Row: centre, c_%d .. c_0%s.  %d bytes.  Worst |1 - E*p - erf| of the double Horner form: %.1e." % (
        degree, ", zero padding to a multiple of 16 B" if row_doubles(degree) != degree + 2 else "", size, worst))
    out.append("#pragma once")
    out.append("namespace fpx {")
    out.append("constexpr int kErfcxIntervals = %d, kErfcxDegree = %d, kErfcxRow = %d;   // kErfcxRow: doubles per row" % (len(rows), degree, row_doubles(degree)))
    out.append("constexpr double kErfcxPerUnit = %d.0, kErfcxMax = %r;" % (per_unit, XMAX))
    out.append("static __device__ const double kErfcxTab[kErfcxIntervals * kErfcxRow] = {")
    for row in rows:
        out.append("  " + ", ".join(float(v).hex() if v != 0.0 else "0.0" for v in row) + ",")
    out.append("};")
    out.append("}  // namespace fpx")
    return "\n".join(out) + "\n"


def main(argv):
    best, report = choose()
    if "--report" in argv:
        print("intervals/unit  degree  intervals  bytes  worst |1 - E*p - erf|")
        for size, per_unit, degree, worst, rows in report:
            print("%14d  %6d  %9d  %5d  %.2e%s" % (per_unit, degree, len(rows), size, worst, "   <- chosen" if (size, per_unit, degree) == best[:3] else ""))
        return 0
    sys.stdout.write(header(best))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
