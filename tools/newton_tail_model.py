#!/usr/bin/env python3
"""CPU model of the refinement steps behind the fp64 root and reciprocal helpers of fpx_device.hpp.

Every helper takes a seed of relative error up to eps0 and refines it, either by two quadratic Newton steps ("q2") or by one
cubic step ("c1").  This model runs both forms in exact IEEE double arithmetic: a product or a sum of two doubles is rounded
once by the host, a fused multiply-add is evaluated in rational arithmetic and rounded once.  The seed is NOT the hardware's: it
is the true value times (1 + d) with d spread over [-eps0, +eps0] (both ends included), rounded to the seed's format (double for
v_rcp_f64 / v_rsq_f64, float for the exp2f(log2f()) seeds).  The result is compared with mpmath at 200 bits and the worst error
is given in units of the last place of the true value.

    python tools/newton_tail_model.py                       # eps0 = 2^-23 (hardware seeds), 2^-19 (f32 seeds), 4000 points
    python tools/newton_tail_model.py --eps-hw -26.5 --eps-f32 -21.3 --points 2000      # log2 of the eps0 to assume

eps0 per seed can be given singly (--eps-rcp, --eps-rsq, --eps-cbrt, --eps-fifth), which is how the measured values of a
device go in.
"""
import argparse
import json
import math
import struct
from fractions import Fraction

import mpmath as mp

mp.mp.prec = 200


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


# ---- the forms, operation for operation as in fpx_device.hpp ----
def rcp_q2(b, r):
    e = fma(-b, r, 1.0)
    r = fma(r, e, r)
    e = fma(-b, r, 1.0)
    return fma(r, e, r)


def rcp_c1(b, r):
    e = fma(-b, r, 1.0)
    t = fma(e, e, e)
    return fma(r, t, r)


def rsqrt_q2(x, y):
    g, h = x * y, 0.5 * y
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    h = fma(h, r, h)
    r = fma(-h, g, 0.5)
    h = fma(h, r, h)
    return h + h


def rsqrt_c1(x, y):
    t = x * y
    e = fma(-t, y, 1.0)
    p = fma(e, 0.375, 0.5)
    return fma(y, e * p, y)


def sqrt_q2(x, y):
    g, h = x * y, 0.5 * y
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    h = fma(h, r, h)
    d = fma(-g, g, x)
    return fma(d, h, g)


def sqrt_c1(x, y):
    g, h = x * y, 0.5 * y
    r = fma(-h, g, 0.5)
    t = fma(r, 1.5, 1.0)
    return fma(g, r * t, g)


def sqrt_rsqrt_q2(x, y):
    g, h = x * y, 0.5 * y
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    h = fma(h, r, h)
    d = fma(-g, g, x)
    g = fma(d, h, g)
    r = fma(-h, g, 0.5)
    h = fma(h, r, h)
    return g, h + h


def sqrt_rsqrt_c1(x, y):
    g, h = x * y, 0.5 * y
    r = fma(-h, g, 0.5)
    rt = r * fma(r, 1.5, 1.0)
    h1 = fma(h, rt, h)
    return fma(g, rt, g), h1 + h1


def rcbrt_q2(x, r):
    for _ in range(2):
        e = fma(-(x * (r * r)), r, 1.0)
        r = fma(r * (1.0 / 3.0), e, r)
    return r


def rcbrt_c1(x, r):
    e = fma(-(x * (r * r)), r, 1.0)
    t = fma(e, 2.0 / 9.0, 1.0 / 3.0)
    return fma(r * e, t, r)


def rfifth_q2(x, r):
    for _ in range(2):
        r2 = r * r
        r5 = (r2 * r2) * r
        e = fma(-x, r5, 1.0)
        r = fma(r * 0.2, e, r)
    return r


def rfifth_c1(x, r):
    r2 = r * r
    r5 = (r2 * r2) * r
    e = fma(-x, r5, 1.0)
    t = fma(e, 0.12, 0.2)
    return fma(r * e, t, r)


def ulps(got, true):
    """|got - true| in units of the last place of the double next to `true` (an mpf)"""
    _, ex = math.frexp(float(true))
    return float(abs(mp.mpf(got) - true) / mp.ldexp(1, ex - 53))


# helper -> (seed, true value as an mpf function of x, seed format, {form: function}, results per call)
HELPERS = {
    "rcp": ("rcp", lambda x: 1 / x, float, {"q2": rcp_q2, "c1": rcp_c1}),
    "rsqrt": ("rsq", lambda x: 1 / mp.sqrt(x), float, {"q2": rsqrt_q2, "c1": rsqrt_c1}),
    "sqrt": ("rsq", mp.sqrt, float, {"q2": sqrt_q2, "c1": sqrt_c1}),
    "sqrt_rsqrt.s": ("rsq", mp.sqrt, float, {"q2": lambda x, y: sqrt_rsqrt_q2(x, y)[0], "c1": lambda x, y: sqrt_rsqrt_c1(x, y)[0]}),
    "sqrt_rsqrt.rs": ("rsq", lambda x: 1 / mp.sqrt(x), float, {"q2": lambda x, y: sqrt_rsqrt_q2(x, y)[1], "c1": lambda x, y: sqrt_rsqrt_c1(x, y)[1]}),
    "rcbrt": ("cbrt", lambda x: mp.root(x, 3) ** -1, f32, {"q2": rcbrt_q2, "c1": rcbrt_c1}),
    "x^-1/5": ("fifth", lambda x: mp.root(x, 5) ** -1, f32, {"q2": rfifth_q2, "c1": rfifth_c1}),
    "pow08": ("fifth", lambda x: mp.root(x, 5) ** 4, f32, {"q2": lambda x, r: x * rfifth_q2(x, r), "c1": lambda x, r: x * rfifth_c1(x, r)}),
}
# what the seed approximates, per seed
SEED_OF = {"rcp": lambda x: 1 / x, "rsq": lambda x: 1 / mp.sqrt(x), "cbrt": lambda x: mp.root(x, 3) ** -1, "fifth": lambda x: mp.root(x, 5) ** -1}
# third-order coefficient C of the cubic step's error C * e0^3 (e0 the seed's relative error), and the e0 at which that is 2^-56
THIRD_ORDER = {"rcp": 1.0, "rsq": 5.0 / 16.0, "sqrt": 0.5, "cbrt": 14.0 / 81.0, "fifth": 0.088}


# the same coefficient with the residual written in the seed's relative error e0: 1 - b*r = e0, 1 - x*y^2 = 2 e0 (5/16 * 2^3; the
# square root's form is the same series in r = e/2), 1 - x*r^3 = 3 e0 (14/81 * 3^3), 1 - x*r^5 = 5 e0 (0.088 * 5^3).  This is the
# step's error in terms of what a seed probe measures, and the one that decides.
THIRD_ORDER_IN_SEED_ERROR = {"rcp": 1.0, "rsq": 2.5, "sqrt": 2.5, "cbrt": 14.0 / 3.0, "fifth": 11.0}


def eps0_bound(c):
    """largest e0 for which c * e0^3 <= 2^-56 (a tenth of an ulp)"""
    return (2.0 ** -56 / c) ** (1.0 / 3.0)


def run(eps=None, points=4000, seed=1):
    """worst error in ulp per helper and form; eps: {"rcp", "rsq", "cbrt", "fifth"} -> eps0"""
    import random
    e0 = {"rcp": 2.0 ** -23, "rsq": 2.0 ** -23, "cbrt": 2.0 ** -19, "fifth": 2.0 ** -19}
    e0.update(eps or {})
    out = {}
    for name, (sd, true_fn, fmt, forms) in HELPERS.items():
        rng = random.Random(seed)
        worst = dict.fromkeys(forms, 0.0)
        for i in range(points):
            x = math.ldexp(1.0 + rng.random(), rng.randrange(-30, 31))
            d = (-1.0, 1.0)[i & 1] * e0[sd] if i % 4 < 2 else rng.uniform(-e0[sd], e0[sd])
            xm = mp.mpf(x)
            y = fmt(float(SEED_OF[sd](xm) * (1 + mp.mpf(d))))
            true = true_fn(xm)
            for form, fn in forms.items():
                worst[form] = max(worst[form], ulps(fn(x, y), true))
        out[name] = worst
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--eps-hw", type=float, default=-23.0, help="log2 of eps0 of v_rcp_f64 and v_rsq_f64")
    ap.add_argument("--eps-f32", type=float, default=-19.0, help="log2 of eps0 of the two f32 seeds")
    for s in ("rcp", "rsq", "cbrt", "fifth"):
        ap.add_argument(f"--eps-{s}", type=float, default=None, help=f"log2 of eps0 of the {s} seed alone")
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    lg = {"rcp": a.eps_hw, "rsq": a.eps_hw, "cbrt": a.eps_f32, "fifth": a.eps_f32}
    for s in lg:
        if getattr(a, f"eps_{s}") is not None:
            lg[s] = getattr(a, f"eps_{s}")
    res = run({s: 2.0 ** v for s, v in lg.items()}, a.points, a.seed)
    if a.json:
        print(json.dumps({"log2_eps0": lg, "points": a.points, "worst_ulp": res}))
        return
    print("seed      log2(eps0)  log2 of the largest eps0 with C*eps0^3 <= 2^-56: C of the series in the residual / C in the seed's error")
    for s, v in lg.items():
        uses = [s] + (["sqrt"] if s == "rsq" else [])
        print(f"{s:9s} {v:9.2f}   " + ", ".join(f"{math.log2(eps0_bound(THIRD_ORDER[u])):.2f} (C = {THIRD_ORDER[u]:.3g}) / {math.log2(eps0_bound(THIRD_ORDER_IN_SEED_ERROR[u])):.2f} (C = {THIRD_ORDER_IN_SEED_ERROR[u]:.3g}) [{u}]" for u in uses))
    print(f"\nworst error in ulp over {a.points} points\nhelper          two quadratic   one cubic")
    for name, w in res.items():
        print(f"{name:15s} {w['q2']:10.2f} {w['c1']:13.2f}")


if __name__ == "__main__":
    main()
