"""The step's invariants of the Langevin kernel (step_invariants, fpx_device.hpp).

A particle's horizontal position is fixed while it is in the Langevin kernel, so h, ol, ust and wst are: k_prep takes what
hanna() / hanna_short() derive from them alone once per particle and the hand-over record carries it.  Moving an exact
computation must not change a bit:
  1. hanna() from the invariants -- taken as in k_prep, packed as the record carries them, read through the stash as in
     k_pbl_loop -- against hanna() as it stands, bitwise, over a grid of (h, ol, ust, wst, z) (fpx_hanna_probe: one launch per
     form).  The probe is not the engine's own call sites: that the contraction there is the parent's is what 2. and the
     byte-identical output dumps of the benchmark stand for;
  2. the engine against the CPU oracle on the scenarios of the parity tests (hanna, cbl, backward_cbl; r8 and r4) at their
     tolerances, with the work-list options that change the order and the launches of the Langevin kernel -- and the particle
     states bitwise equal across those options (a resumed particle takes its invariants at the refill, not from k_prep);
  3. runs with ldirect = -1 (timedir is a sign mask in cbl()) through the same comparison;
  4. turbswitch off with ifine > 1: hanna1 at the head of the pass, hanna_short after every sub-step but the last
     (advance.f90:493-495) -- the one path on which both read the surface-layer scales.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from flexpart_amd import synthetic as syn

pytestmark = pytest.mark.gpu

STATE = ("xtra1", "ytra1", "ztra1", "uap", "ucp", "uzp", "us", "vs", "ws", "idt", "itra1", "cbt", "xmass1")
COLS = ("sigu", "sigv", "sigw", "dsigwdz", "1/tlu", "1/tlv", "tlw", "ust", "regime", "cbl_on")


def hanna_probe(points):
    from flexpart_amd import _lib
    lib = _lib.load()
    x = np.ascontiguousarray(points, np.float64)
    assert x.ndim == 2 and x.shape[1] == 5
    y = np.empty((2, x.shape[0], 10), np.float64)
    rc = lib.fpx_hanna_probe(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.shape[0])
    assert rc == 0
    return y[0], y[1]


def test_hanna_from_the_invariants_is_hanna_bit_for_bit(built):
    rng = np.random.default_rng(5)
    pts = []
    hs = (80.0, 400.0, 1234.5, 2600.0)
    # h/|ol| on both sides of 1 (neutral | not) and -h/ol on both sides of 5 (the skewed CBL scheme), ol of both signs
    ratios = (0.02, 0.5, 1.0 - 1e-12, 1.0, 1.0 + 1e-12, 2.0, 5.0 - 1e-12, 5.0, 5.0 + 1e-12, 9.0, 15.0, 80.0, 3000.0)
    usts = (1e-6, 5e-5, 1e-4 * (1 - 1e-15), 1e-4, 1e-4 * (1 + 1e-15), 3e-3, 0.08, 0.35, 1.4)
    wsts = (0.0, 0.2, 1.1, 3.0)
    zetas = (0.0, 1e-40, 1e-4, 1e-3, 1e-3 * (1 + 1e-15), 0.03, 0.1 * (1 - 1e-15), 0.1, 0.4, 0.99, 1.0)
    for h, r, sgn, ust, wst, zeta in itertools.product(hs, ratios, (-1.0, 1.0), usts, wsts, zetas):
        pts.append((h, sgn * h / r, ust, wst, zeta * h))
    n = 200000
    h = rng.uniform(50.0, 3000.0, n)
    ol = rng.choice([-1.0, 1.0], n) * h / np.exp(rng.uniform(np.log(0.05), np.log(500.0), n))
    pts = np.concatenate([np.array(pts), np.stack([h, ol, np.exp(rng.uniform(np.log(1e-5), np.log(2.0), n)), rng.uniform(0.0, 3.0, n),
                                                   h * rng.uniform(0.0, 1.0, n)], axis=1)])
    inv, ref = hanna_probe(pts)
    # every case the grid is there for did occur
    assert set(np.unique(ref[:, 8])) == {0.0, 1.0, 2.0} and set(np.unique(ref[:, 9])) == {0.0, 1.0}
    floored = ref[:, 7] != pts[:, 2]
    assert floored.any() and (~floored).any() and np.all(ref[floored, 8] == 0.0)
    for j, name in enumerate(COLS):
        a, b = inv[:, j].copy().view(np.uint64), ref[:, j].copy().view(np.uint64)
        diff = np.flatnonzero(a != b)
        assert diff.size == 0, f"{name}: {diff.size} of {len(pts)} points differ, first at (h, ol, ust, wst, z) = {pts[diff[0]]}: {inv[diff[0], j]!r} != {ref[diff[0], j]!r}"


def _scenario(name):
    if name == "hanna_backward":
        return syn.small(n=3000, nx=40, ny=24, nz=30, nsteps=3, ctl=5.0, ifine=4, ldirect=-1)
    from test_oracle_cpu import golden_scenario
    return golden_scenario(name)


OPTIONS = ({"pbl_cost_buckets": 0}, {"pbl_cost_buckets": 3}, {"pbl_slices": "1,2,5,0"})


@pytest.mark.parametrize("kind", ["r8", "r4"])
@pytest.mark.parametrize("name", ["hanna", "cbl", "backward_cbl", "hanna_backward"])
def test_engine_matches_oracle_under_every_schedule(built, name, kind):
    """hanna / cbl / backward_cbl: the scenarios of test_fp64_matches_oracle_golden_scenarios and of
    test_reference_typed_f32_cbl_against_reference_fixtures, at their tolerances; backward_cbl and hanna_backward run with
    ldirect = -1.  pbl_slices 1,2,5,0 suspends nearly every particle several times: it then takes its invariants at the
    refill of the next launch, from the same helper."""
    from test_gpu_parity import assert_close, run_pair
    sc = _scenario(name)
    n = int(sc["npart"])
    ref = None
    for opt in OPTIONS:
        got, want = run_pair(sc, kind, options=dict(opt))
        for g, w in zip(got, want):
            if kind == "r8":
                assert_close(g, w, 1e-9, 1e-7)
            else:
                assert_close(g, w, 2e-6, 5e-3, max_diverged=int(0.02 * n))
        if ref is None:
            ref = got
            continue
        for a, b in zip(ref, got):
            for k in STATE:
                assert np.array_equal(a[k], b[k]), (opt, k)


@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_hanna1_with_fine_sub_steps(built, kind):
    """turbswitch = 0 and ifine = 4 (readcommand.f90 sets ifine = 1 with ctl < 0, so the scenario is switched by hand; the
    engine accepts it): hanna1 reads wst itself, hanna_short of sub-steps 1 to ifine - 1 reads wst*wst from the stash."""
    from test_gpu_parity import assert_close, run_pair
    sc = syn.small(n=4000, nx=60, ny=40, nz=40, nsteps=3, ctl=-5.0)
    assert int(sc["turbswitch"]) == 0 and int(sc["ifine"]) == 1
    sc["ifine"] = 4
    n = int(sc["npart"])
    ref = None
    for opt in OPTIONS:
        got, want = run_pair(sc, kind, options=dict(opt))
        for g, w in zip(got, want):
            if kind == "r8":
                assert_close(g, w, 1e-9, 1e-7)
            else:
                assert_close(g, w, 2e-6, 5e-3, max_diverged=int(0.02 * n))
        assert np.abs(got[-1]["uzp"]).max() > 0
        if ref is None:
            ref = got
            continue
        for a, b in zip(ref, got):
            for k in STATE:
                assert np.array_equal(a[k], b[k]), (opt, k)
