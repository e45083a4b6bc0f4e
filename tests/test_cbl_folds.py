"""cbl() after its rounding-level folds and with the table-driven error-function pair: the engine against the CPU oracle.

The fp64 gas kernels of the Langevin loop read the error-function pair of cbl.f90:195-204 from a piecewise table in LDS, the
fp64 aerosol kernels keep the polynomial form (their stash leaves no room), and both run the folded arithmetic of cbl()
(fpx_device.hpp).  The cloud is the CBL recipe of the golden scenarios with 6000 particles and ifine = 11 (what readcommand.f90
sets for cblflag = 1 at ctl = 5), three steps, on a column of 138 levels and on the shortest one that has a level pair above
the ground (nz = 3), once as a gas and once as an aerosol species, and once backward in time.

That the recipe reaches cbl() at all is pinned from its fields (in_cbl_columns): more than a twentieth of the cloud starts
below the mixing height in cells whose four corners have -h/L > 5.

Tolerances: those of the fp64 CBL cases of tests/test_gpu_parity.py, with no diverged particle.  That file states them as
literals in its calls of assert_close; test_tolerances_are_those_of_the_parity_tests holds the pair below to them.
"""
import functools

import numpy as np
import pytest

from flexpart_amd import synthetic as syn

TOL_POS, TOL_VEL = 1e-9, 1e-7
N, IFINE, NSTEPS = 6000, 11, 3


def test_tolerances_are_those_of_the_parity_tests():
    import test_gpu_parity as tp
    for fn in (tp.test_fp64_matches_oracle, tp.test_fp64_matches_oracle_golden_scenarios):
        assert {TOL_POS, TOL_VEL} <= set(fn.__code__.co_consts), fn.__name__


@functools.lru_cache(maxsize=None)
def scenario(species, nz, ldirect):
    from test_oracle_cpu import CASES, _aerosol
    kw = dict(CASES["cbl"], ifine=IFINE)
    sc = syn.small(n=N, nx=48, ny=32, nz=nz, nsteps=NSTEPS, ldirect=ldirect, **kw)
    assert int(sc["cblflag"]) == 1 and int(sc["ifine"]) == IFINE and len(sc["height"]) == nz
    return _aerosol(sc) if species == "aerosol" else sc


def in_cbl_columns(sc):
    """Particles that start below the mixing height in a cell whose four corners have -h/L > 5 at the first wind-field time,
    where the run starts (three steps are a small part of the interval to the second): the condition under which
    advance.f90:405 calls cbl(), whatever the interpolation makes of h and L inside such a cell."""
    deep = -np.asarray(sc["hmix"])[0] * np.asarray(sc["oli"])[0] > 5.0
    hmin = np.asarray(sc["hmix"])[0]
    ix, jy = np.asarray(sc["xtra1"]).astype(int), np.asarray(sc["ytra1"]).astype(int)
    ok = np.ones(len(ix), bool)
    for dj in (0, 1):
        for di in (0, 1):
            j, i = np.minimum(jy + dj, deep.shape[0] - 1), (ix + di) % deep.shape[1]
            ok &= deep[j, i] & (np.asarray(sc["ztra1"]) < hmin[j, i])
    return ok


def test_the_recipe_reaches_the_scheme():
    for key in (("gas", 138, 1), ("gas", 3, 1), ("aerosol", 138, 1), ("aerosol", 3, 1), ("gas", 138, -1)):
        assert in_cbl_columns(scenario(*key)).mean() > 0.05, key


@pytest.mark.gpu
@pytest.mark.parametrize("species,nz,ldirect", [("gas", 138, 1), ("gas", 3, 1), ("aerosol", 138, 1), ("aerosol", 3, 1), ("gas", 138, -1)])
def test_cbl_against_the_oracle(built, species, nz, ldirect):
    from test_gpu_parity import assert_close, run_pair
    sc = scenario(species, nz, ldirect)
    got, want = run_pair(sc, "r8")
    assert len(got) == NSTEPS
    for g, w in zip(got, want):
        assert assert_close(g, w, TOL_POS, TOL_VEL, max_diverged=0) == 0
    # the cloud moved, and the recipe still reaches cbl() itself
    moved = got[-1]["ztra1"] != np.asarray(sc["ztra1"])
    assert moved.mean() > 0.5
    assert in_cbl_columns(sc).mean() > 0.05
