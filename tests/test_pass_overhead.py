"""What a Langevin pass does around its fine sub-steps (pbl_pass, fpx_device.hpp), after the per-pass work was cut:

  * the level search starts from the level the lane found in its previous pass (find_level_from): tested, walked by up to two
    levels, then the bisection.  The refill hands it the level k_prep found for the particle's height;
  * in the unstable regime, where 1/tlv is 1/tlu, the pair of factors of the horizontal Langevin step is taken once.

Both are exact: no output bit may change.

  1. fpx_find_level_probe: the search from every possible guess against the plain bisection -- the level and the two heights the
     pass reads after it, bitwise, fp64 and f32 -- on columns of nz = 2, 3, 30 and 138, for z on every level, one ulp either
     side of it, 0, below the column, just under its top, above it, and not a number.  The plain search itself is held to
     numpy's searchsorted.
  2. the engine against the CPU oracle (fp64, serial-stream RNG, the tolerances of tests/test_step_invariants.py) and, fp64 and
     f32, serial-stream and counter RNG, the narrow schedules of tests/test_schedule_parity.py against the default one bit for
     bit, on the oracle scenarios of tests/test_step_invariants.py with ctl = 5 and ctl = -5 (one pass of lsynctime: dt/tlu >= .5,
     the exponential form of the horizontal step) and ifine = 1, 4 and 11 (the counter RNG's last block of a pass is read up
     to its fourth, third and second normal).  ctl = -5 switches hanna() off (readcommand.f90), so one more case runs
     ctl = -5 with turbswitch set by hand: the exponential form in the unstable regime, where the factors are shared.
  3. the cold path of the CBL scheme (re_initialize_particle, which draws beyond the pass's own random numbers) did run in an
     fp64 CBL case: the engine's nan_count is not zero.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from flexpart_amd import synthetic as syn

pytestmark = pytest.mark.gpu

STATE = ("xtra1", "ytra1", "ztra1", "uap", "ucp", "uzp", "us", "vs", "ws", "idt", "itra1", "cbt", "xmass1")


# ---- 1. the level search ---------------------------------------------------------------------------------------------------------

def column(nz, dtype):
    """nz strictly increasing heights from 0, stretched like the model's levels."""
    return np.concatenate([[0.0], np.cumsum(12.5 * 1.045 ** np.arange(nz - 1))]).astype(dtype)


def probe_points(hgt):
    """(z, guess) pairs: every z of the docstring with every guess 0 .. nz-1 and three values that are no level."""
    dt = hgt.dtype.type
    nz = len(hgt)
    inf = dt(np.inf)
    z = [hgt, np.nextafter(hgt, -inf), np.nextafter(hgt, inf),
         np.array([0.0, -0.0, -1.0, hgt[-1] - dt(100.0) * np.finfo(dt).eps, hgt[-1] + dt(10.0), 0.5 * (hgt[0] + hgt[1]), np.nan], dt)]
    z = np.concatenate(z).astype(dt)
    guess = np.concatenate([np.arange(0, nz), [-1, nz, nz + 5]]).astype(np.int32)
    zz, gg = np.meshgrid(z, guess, indexing="ij")
    return np.ascontiguousarray(zz.ravel()), np.ascontiguousarray(gg.ravel())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nz", [2, 3, 30, 138])
def test_level_search_from_a_guess_is_the_plain_search(built, nz, dtype):
    from flexpart_amd import _lib
    lib = _lib.load()
    hgt = column(nz, dtype)
    assert np.all(np.diff(hgt) > 0)
    z, guess = probe_points(hgt)
    n = z.size
    idx = np.full((2, n), -7, np.int32)
    hh = np.full((2, n, 2), -7.0, dtype)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.fpx_find_level_probe(hgt.itemsize, p(hgt), nz, p(z), p(guess), n, p(idx), p(hh))
    assert rc == 0
    # the plain search: first level above z, clamped to the column (NaN compares false everywhere: the top pair)
    want = np.clip(np.searchsorted(hgt[1:], z, side="right") + 1, 1, nz - 1)
    want[np.isnan(z)] = nz - 1
    assert np.array_equal(idx[1], want)
    assert np.array_equal(hh[1, :, 0], hgt[want - 1]) and np.array_equal(hh[1, :, 1], hgt[want])
    # every level was an answer, and guesses on both sides of it and farther than the walk were tried
    assert set(np.unique(want)) == set(range(1, nz))
    if nz > 6:
        off = guess - want
        assert off.min() < -3 and off.max() > 3
    bad = np.flatnonzero(idx[0] != idx[1])
    assert bad.size == 0, f"{bad.size} of {n}: z = {z[bad[0]]!r}, guess {guess[bad[0]]}: {idx[0, bad[0]]} != {idx[1, bad[0]]}"
    ut = np.uint64 if dtype is np.float64 else np.uint32
    assert np.array_equal(hh[0].view(ut), hh[1].view(ut))


# ---- 2. / 3. the engine ----------------------------------------------------------------------------------------------------------

NAMES = ("hanna", "cbl", "backward_cbl", "hanna_backward")
# the narrow schedules of tests/test_schedule_parity.py (one block: every wave refills many times; list order, slot order, time slices)
SCHEDULES = {
    "default": {},
    "narrow_list": {"pbl_cost_buckets": 0, "pbl_grid_blocks": 1, "finish_blocks": 1},
    "narrow_slots": {"pbl_cost_buckets": 3, "pbl_grid_blocks": 1, "finish_blocks": 1},
    "narrow_sliced": {"pbl_cost_buckets": 0, "pbl_grid_blocks": 1, "finish_blocks": 1, "pbl_slices": "1,2,5,0", "pbl_drain_lanes": 32},
}


@functools.lru_cache(maxsize=None)
def scenario(name, ctl, ifine, turbswitch=None):
    """The scenario `name` of tests/test_step_invariants.py with another ctl and, set by hand as test_hanna1_with_fine_sub_steps
    does, ifine (readcommand.f90 would raise it to 11 with cblflag = 1 and set 1 with ctl < 0) and turbswitch."""
    decay = name.endswith("_decay")
    name = name[:-len("_decay")] if decay else name
    if name == "hanna_backward":
        sc = syn.small(n=3000, nx=40, ny=24, nz=30, nsteps=3, ctl=ctl, ifine=ifine, ldirect=-1)
    else:
        from test_oracle_cpu import CASES
        kw = dict(CASES[name], ctl=ctl, ifine=ifine)
        assert "post" not in kw and "grid" not in kw
        sc = syn.small(n=1500, nx=48, ny=32, nz=36, nsteps=3, **kw)
    sc["ifine"] = ifine
    if decay:
        # ust and wst fall to a twentieth over four steps (the second wind-field time is the end of the fourth): a particle then
        # carries a wp of the step before into turbulence a third as strong, beyond 6 sigma of both Gaussians of cbl.f90
        ld = int(sc["ldirect"])
        for k in ("ustar", "wstar"):
            f = np.array(sc[k])
            f[1] = 0.05 * f[0]
            sc[k] = f
        sc["memtime"] = np.array([0, 2700 * ld], np.int32)
        sc["nsteps"] = 4
    if turbswitch is not None:
        sc["turbswitch"] = turbswitch
    return sc


def run_engine(sc, rb, mode, options):
    from flexpart_amd.engine import Engine
    eng = Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=mode, seed=77, options=dict(options))
    got = eng.run()
    counters = eng.counters()
    eng.close()
    return got, counters


@functools.lru_cache(maxsize=None)
def check_case(name, ctl, ifine, turbswitch=None):
    """Oracle once; fp64 and f32, both RNG modes, every schedule.  -> the nan_count of the fp64 serial-stream default run."""
    sc = scenario(name, ctl, ifine, turbswitch)
    from flexpart_amd.engine import RNG_PHILOX, RNG_TABLE_SEQ
    from oracle.oracle import Oracle
    from test_gpu_parity import assert_close
    orc = Oracle(sc, "r8")
    orc.lib.orc_set_parallel_semantics(orc.h, 1)
    want = orc.run()
    nan_count = None
    orc_nan = int(orc.nan_counts()[0])
    for rb in (8, 4):
        for mode in (RNG_TABLE_SEQ, RNG_PHILOX):
            ref = None
            for sched, options in SCHEDULES.items():
                got, counters = run_engine(sc, rb, mode, options)
                assert counters["n_bad_position"] == 0
                if rb == 8 and mode == RNG_TABLE_SEQ:
                    for g, w in zip(got, want):
                        assert_close(g, w, 1e-9, 1e-7)
                if ref is None:
                    ref = got
                    if rb == 8 and mode == RNG_TABLE_SEQ:
                        nan_count = counters["nan_count"]
                        assert nan_count == orc_nan, (nan_count, orc_nan)
                    assert (got[-1]["ztra1"] != np.asarray(sc["ztra1"])).mean() > 0.5      # the cloud did move
                    continue
                for a, b in zip(ref, got):
                    for k in STATE:
                        assert np.array_equal(a[k], b[k], equal_nan=True), (rb, mode, sched, k)
    return nan_count


@pytest.mark.parametrize("ifine", [1, 4, 11])
@pytest.mark.parametrize("ctl", [5.0, -5.0])
@pytest.mark.parametrize("name", NAMES)
def test_step_parity(built, name, ctl, ifine):
    sc = scenario(name, ctl, ifine)
    assert int(sc["ifine"]) == ifine
    if ctl < 0 and not int(sc["cblflag"]):
        assert int(sc["turbswitch"]) == 0 and abs(int(sc["mintime"])) == abs(int(sc["lsynctime"]))
    check_case(name, ctl, ifine)


@pytest.mark.parametrize("name", ["hanna", "hanna_backward"])
def test_step_parity_exponential_form_with_hanna(built, name):
    """ctl = -5 (method 0: one pass of dt = lsynctime = 900 s, so dt/tlu >= .5 wherever tlu <= 1800 s) with hanna() switched on
    by hand: the exponential form of the horizontal step in the unstable regime, where its factors are taken once for u and v."""
    sc = scenario(name, -5.0, 4, turbswitch=1)
    assert int(sc["method"]) == 0 and int(sc["turbswitch"]) == 1
    check_case(name, -5.0, 4, 1)


def test_cold_cbl_path_ran(built):
    """re_initialize_particle (cbl.f90's flagrein) draws past the random numbers a pass expects to read; the engine counts those
    events in nan_count (fp64, serial-stream RNG, default schedule; check_case holds it to the oracle's count).  On the CPU
    oracle no committed scenario reaches that path, and neither do the seeds 1 .. 12 of the CBL recipe at 6000 particles, forward
    or backward; with ust and wst decaying to a twentieth over four steps (scenario(): "_decay") some tens of particles do.

    ifine = 11 only, the value readcommand.f90 sets for cblflag = 1 at ctl = 5 (ifine*ctl >= 50).  With ifine = 4 the decaying
    cloud is no case for the oracle's tolerances: two particles blow up in the Gaussian arm (the oracle's second counter, the
    non-finite wp of advance.f90:440, is 2), and the CPU oracle run against ITSELF with ustar, wstar or hmix scaled by
    1 +- 2.3e-16 ends with those two of 1500 particles beyond 1e-9 / 1e-7 in steps 3 and 4 (1 or 2 in each of the six
    perturbed runs).  With ifine = 11 that counter is 0 and all six perturbed oracle runs stay within the tolerances."""
    counts = {(name, ifine): check_case(name, 5.0, ifine) for name in ("cbl_decay", "backward_cbl_decay") for ifine in (11,)}
    print("[cold CBL path] nan_count per (scenario, ifine):", counts)
    assert max(counts.values()) > 0, counts
