"""Bounds for the device's convection matrices, computed from the reference side alone (tests/test_convection.py).

The device computes the scheme in the reference's order of operations with FMA contraction off; what can differ from the
CPU result is libm (exp, log, pow) and the order of the O(levels^2) FUP / FDOWN sums of the level-parallel kernels.  The
oracle routes every libm result through one function that can move it by a whole number of ulps of the real kind
(oracle/convect_oracle.c: cvo_set_libm_perturbation), so how far a different libm that keeps a 1-ulp bound may move each
result is measured on the oracle: five perturbed runs (three random seeds from {-2 .. +2} ulp, all +2, all -2; 2 ulp = the
1 ulp of glibc plus the 1 ulp of the device library) against the unperturbed one.

  B_fm[c]   = max(8 * max over the runs of max |d fmassfrac| of column c,  4 * ulp_H(max |fmassfrac| of column c))
  B_uvz[c]  the same for uvzlev(1 .. nconvtop+1)
  cb_bound  the same for the whole cbaseflux field (cbasefluxn), per call, as an absolute bound

The factor 8 covers what the perturbation does not model: the re-ordered sums, and that five runs are a sample, not the
worst case.  The bounds hold for a case only while no perturbation changes lconv or nconvtop of any column (`noflip`),
which a CPU test asserts for every case the GPU tests use.  No constant is committed: everything is computed at test time
(six oracle runs, about a second) and shared between the tests of a session."""
import numpy as np

from oracle.oracle import LIBM_DOWN, LIBM_RANDOM, LIBM_UP, conv_oracle

PERTURBATIONS = ((LIBM_RANDOM, 101), (LIBM_RANDOM, 202), (LIBM_RANDOM, 303), (LIBM_UP, 0), (LIBM_DOWN, 0))
FACTOR, FLOOR_ULPS = 8.0, 4.0
HEIGHT_TOL = {"r8": 1e-9, "r4": 2e-4}          # relative tolerance of a particle height (max(|z|, 1) as the scale)

_cache = {}


def ulp(x, kind):
    """Spacing of the real kind at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32 if kind == "r4" else np.float64)).astype(np.float64)


def ncolumns(cs):
    nx, ny, _ = (int(v) for v in cs["grid"])
    return nx * ny + (int(cs["nest"][0]) * int(cs["nest"][1]) if "nest" in cs else 0)


def all_columns(call, cs):
    """lconv and nconvtop of every column in the engine's numbering (mother grid, then the nest)."""
    lc, nt = call["lconv"].ravel(), call["nconvtop"].ravel()
    if "nest" in cs:
        lc, nt = np.concatenate([lc, call["lconvn"].ravel()]), np.concatenate([nt, call["nconvtopn"].ravel()])
    return lc, nt


def outside(z, zref, kind):
    """Particles whose height is outside the tolerance."""
    return np.abs(z - zref) > HEIGHT_TOL[kind] * np.maximum(np.abs(zref), 1.0)


def _bound(dev, scale, kind):
    return np.maximum(FACTOR * dev, FLOOR_ULPS * ulp(scale, kind))


def reference(key, cs, kind):
    """The oracle on the case cs (with height_nz set), unperturbed and under PERTURBATIONS.  -> dict:
    calls      the unperturbed result of every call, matrices and half-level heights of all convective columns recorded
    cols       [m] engine numbers of the convective columns of the first call, in the order of calls[0]["fmassfrac"]
    B_fm, B_uvz [m] the bounds above, first call
    cb_bound, cbn_bound  [ncalls] absolute bounds of cbaseflux / cbasefluxn after each call
    noflip     no perturbation changed lconv or nconvtop of a column, in any call
    worst_outside  particles outside the height tolerance after the first call, worst perturbed run
    dev_fm, dev_uvz, dev_cb  the largest deviations the perturbations produced (for the record)"""
    k = (key, kind)
    if k in _cache:
        return _cache[k]
    cap = ncolumns(cs)
    dim = int(cs["nconvlev"]) + 1                  # nconvtop reaches nconvlev + 1
    base = conv_oracle(cs, kind, fm_cap=cap, fm_dim=dim)
    b0 = base[0]
    m = b0["fm_count"]
    cols = b0["fm_col"][:m].copy()
    fm0, uz0 = b0["fmassfrac"][:m], b0["uvzlev"][:m]
    dfm, duz = np.zeros(m), np.zeros(m)
    dcb, dcbn = np.zeros(len(base)), np.zeros(len(base))
    noflip, worst = True, 0
    for mode, seed in PERTURBATIONS:
        run = conv_oracle(cs, kind, fm_cap=cap, fm_dim=dim, libm=(mode, seed))
        for ic, (r, b) in enumerate(zip(run, base)):
            lr, tr = all_columns(r, cs)
            lb, tb = all_columns(b, cs)
            noflip = noflip and np.array_equal(lr, lb) and np.array_equal(tr, tb)
            dcb[ic] = max(dcb[ic], np.abs(r["cbaseflux"] - b["cbaseflux"]).max())
            if "nest" in cs:
                dcbn[ic] = max(dcbn[ic], np.abs(r["cbasefluxn"] - b["cbasefluxn"]).max())
        r0 = run[0]
        if r0["fm_count"] == m and np.array_equal(r0["fm_col"][:m], cols):
            if m:
                dfm = np.maximum(dfm, np.abs(r0["fmassfrac"][:m] - fm0).reshape(m, -1).max(axis=1))
                duz = np.maximum(duz, np.abs(r0["uvzlev"][:m] - uz0).max(axis=1))
        else:
            noflip = False
        worst = max(worst, int(outside(r0["ztra1"], b0["ztra1"], kind).sum()))
    out = dict(calls=base, cols=cols, noflip=bool(noflip), worst_outside=worst,
               B_fm=_bound(dfm, np.abs(fm0).reshape(m, -1).max(axis=1) if m else np.zeros(0), kind),
               B_uvz=_bound(duz, np.abs(uz0).max(axis=1) if m else np.zeros(0), kind),
               cb_bound=np.array([_bound(dcb[ic], np.abs(b["cbaseflux"]).max(), kind) for ic, b in enumerate(base)]),
               cbn_bound=np.array([_bound(dcbn[ic], np.abs(b["cbasefluxn"]).max(), kind) if "nest" in cs else 0.0 for ic, b in enumerate(base)]),
               dev_fm=dfm, dev_uvz=duz, dev_cb=dcb)
    _cache[k] = out
    return out


def height_cap(ref):
    """How many particles may be outside the height tolerance after one call: a particle whose random number lies within the
    rounding of a cumulative row sum lands in another level under any other libm too."""
    return max(3, 4 * ref["worst_outside"])
