"""The full-size schedule of the particle step, on clouds the CPU oracle can judge.

Which variant of the step runs depends on the size of the cloud (Engine::step, k_pbl_loop, k_pbl_finish): the order of the work list
("pbl_cost_buckets": 3 below 5e7 particles, 0 from there), the order of k_pbl_finish (list order with buckets 0 -- including the
deferred dry-deposition scatter with a partly filled last wave --, slot order with the per-wave queue otherwise), whether a wave of
k_pbl_finish walks more than one tile (its grid is capped at 8192 blocks; only then does the queue carry move anything), whether a
persistent wave of the Langevin kernel refills PART of its lanes (only when the list is longer than the grid), and the time-blended
wind packs (from 3e7 particles).  A cloud of a few thousand particles takes the small-cloud variant of each.  Here the options
"pbl_cost_buckets", "pbl_grid_blocks" and "finish_blocks" (and blend_mode) make such a cloud take the full-size ones:

* against the oracle in fp64, every schedule, every step, at the tolerances of test_fp64_matches_oracle_golden_scenarios;
* bit for bit across the schedules, fp64 and f32, serial-stream and counter RNG: scheduling must not change a result;
* the concentration and deposition grids against the oracle's at the tolerances of test_conccalc_and_dry_deposition_grids;
* every narrow case proves from the engine's own counters that it reached the path (several chunks per wave, several tiles per wave);
* the ends of the work list (clouds of 1 .. 1000 particles, lists shorter than the cloud, all particles in one stability class);
* at 2.5e6 particles, where the uncapped grids of both kernels bind and no oracle runs: the three full-size schedules bit for bit,
  and a slice of 4096 particle numbers run alone (the size the oracle checks) ends where those particles end in the big run.

The golden scenarios hold 1500 particles, about 750 of them in the boundary layer: three chunks of 64 per wave of ONE block, short
of the eight the narrow cases must prove.  The narrow schedules therefore run those scenarios' own recipe with 6000 particles
(`golden_like`), each against an oracle run and a default-schedule run of the same cloud; the other schedules run the fixtures'
clouds as they are.
"""
import functools

import numpy as np
import pytest

from flexpart_amd import synthetic as syn

pytestmark = pytest.mark.gpu

POS = ("xtra1", "ytra1", "ztra1")
DEAD = -999999999
SEED = 77

CBL = dict(n=4000, nx=60, ny=40, nz=40, nsteps=3, ctl=5.0, ifine=4, cblflag=1, frac_pbl=1.0)


def golden_like(name, n):
    """The recipe of test_oracle_cpu.golden_scenario(name) with n particles instead of 1500."""
    from test_oracle_cpu import CASES
    kw = dict(CASES[name])
    post = kw.pop("post", None)
    nx, ny, nz = kw.pop("grid", (48, 32, 36))
    sc = syn.small(n=n, nx=nx, ny=ny, nz=nz, nsteps=3, **kw)
    return post(sc) if post else sc


def _golden(name, n):
    from test_oracle_cpu import golden_scenario
    sc = golden_scenario(name) if n is None else golden_like(name, n)
    return syn.add_outgrid(sc) if name == "aerosol" else sc


SCENARIOS = {
    "cbl_gas": lambda n: syn.small(**CBL),
    "hanna_gas": lambda n: syn.small(**dict(CBL, cblflag=0)),
    "hanna_backward": lambda n: syn.small(**dict(CBL, cblflag=0, ldirect=-1)),
    "aerosol_outgrid": lambda n: _golden("aerosol", n),
    "nest_wet": lambda n: _golden("nest_wet", n),
    "polar": lambda n: _golden("polar", n),
}
SYN_SMALL = ("cbl_gas", "hanna_gas", "hanna_backward")
WITH_GRIDS = ("aerosol_outgrid", "nest_wet")
NARROW_N = 6000      # particles of the golden recipes under the narrow schedules (see the module's docstring)

# name -> (options, constructor arguments)
SCHEDULES = {
    "default": ({}, {}),
    "buckets0": ({"pbl_cost_buckets": 0}, {}),
    "buckets1": ({"pbl_cost_buckets": 1}, {}),
    "buckets2": ({"pbl_cost_buckets": 2}, {}),
    "as_benched": ({"pbl_cost_buckets": 0}, {"blend_mode": 1}),
    "narrow_list": ({"pbl_cost_buckets": 0, "pbl_grid_blocks": 1, "finish_blocks": 1}, {}),
    "narrow_slots": ({"pbl_cost_buckets": 3, "pbl_grid_blocks": 1, "finish_blocks": 1}, {}),
    "narrow_sliced": ({"pbl_cost_buckets": 0, "pbl_grid_blocks": 1, "finish_blocks": 1, "pbl_slices": "1,2,5,0", "pbl_drain_lanes": 32}, {}),
}
NARROW = ("narrow_list", "narrow_slots", "narrow_sliced")
BITWISE = tuple(s for s in SCHEDULES if s != "as_benched")


def cloud_of(scn, sched):
    """The size key of the cloud a (scenario, schedule) pair runs on: None = the scenario as it stands."""
    return NARROW_N if (sched in NARROW and scn not in SYN_SMALL) else None


@functools.lru_cache(maxsize=None)
def scenario(scn, n=None):
    return SCENARIOS[scn](n)


def _grids_of(obj, sc):
    """Every output grid the scenario has, by name, as float64 arrays of the oracle's shapes."""
    out = {}
    if "outgrid" not in sc:
        return out
    out["gridunc"], out["drygridunc"] = obj.grids()
    if int(sc.get("wetdep", 0)):
        out["wetgridunc"] = obj.wetgrid()
    if "outgridn" in sc:
        out["griduncn"], out["drygriduncn"], out["wetgriduncn"] = obj.grids_nest()
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(scn, n, kind):
    """One oracle run per (scenario, cloud, kind): the states after every step and the grids at the end."""
    from oracle.oracle import Oracle
    sc = scenario(scn, n)
    orc = Oracle(sc, kind)
    orc.lib.orc_set_parallel_semantics(orc.h, 1)
    states = orc.run()
    return states, _grids_of(orc, sc)


@functools.lru_cache(maxsize=None)
def engine_run(scn, sched, rb, mode, n):
    """One engine run per (scenario, schedule, precision, RNG mode, cloud): the states after every step, the grids at the end, and
    what the engine reports about the schedule it ran."""
    from flexpart_amd.engine import Engine
    sc = scenario(scn, n)
    options, ekw = SCHEDULES[sched]
    eng = Engine(sc, compute_real_bytes=rb, host_real_bytes=rb, rng_mode=mode, seed=SEED, options=options, **ekw)
    states, lengths, stats = [], [], []
    for _ in range(int(sc["nsteps"])):
        if eng.has_wet and eng.itime != 0:      # wetdepo first, as Engine.run and the time manager order them
            eng.wetdepo()
        stats.append(eng.step())
        lengths.append(eng.info("pbl_list_length"))
        if eng.gshape is not None:
            eng.conccalc(eng.itime, 1.0)
        states.append(eng.download())
    grids = _grids_of(eng, sc)
    rep = dict(pbl_grid=eng.info("pbl_grid"), launches=eng.info("pbl_launches_per_step"), blended_steps=eng.info("blended_steps"),
               lengths=lengths, stats=stats, numpart=int(sc["npart"]), counters=eng.counters())
    eng.close()
    return states, grids, rep


def assert_reached(scn, sched, rep):
    """The schedule did what its name says -- from the engine's own numbers, nothing hard-coded."""
    options = SCHEDULES[sched][0]
    assert rep["counters"]["n_bad_position"] == 0
    if sched == "as_benched":
        assert rep["blended_steps"] == len(rep["lengths"])
    else:
        assert rep["blended_steps"] == 0
    if sched not in NARROW:
        return
    blocks = options["finish_blocks"]
    assert rep["pbl_grid"] == options["pbl_grid_blocks"] == 1
    waves = rep["pbl_grid"] * 4
    for length in rep["lengths"]:
        # at least 8 chunks of 64 per wave of the capped grid: every wave refills partly busy, many times
        assert length >= 8 * 64 * waves, (scn, sched, length, waves)
    # every wave of k_pbl_finish walks several tiles / strides: in slot order the queue carry runs
    assert rep["numpart"] > 2 * 64 * 4 * blocks, (scn, sched, rep["numpart"])
    if sched == "narrow_sliced":
        assert rep["launches"] == 4


def assert_close(got, want, tol_pos, tol_vel):
    """tests/test_gpu_parity.py::assert_close with no diverged particle allowed: L-inf relative to each field's range, integer
    state equal."""
    n = len(want["xtra1"])
    bad = np.zeros(n, bool)
    for k in ("idt", "itra1", "cbt"):
        bad |= np.asarray(got[k]) != np.asarray(want[k])
    worst = {}
    for keys, tol in ((POS, tol_pos), (("uap", "ucp", "uzp", "us", "vs", "ws"), tol_vel)):
        for k in keys:
            scale = max(np.abs(want[k]).max(), 1e-30)
            err = np.abs(got[k] - want[k]) / scale
            worst[k] = float(err.max()) if n else 0.0
            bad |= err > tol
    assert bad.sum() == 0, f"{bad.sum()} of {n} particles diverged; worst: {worst}"


def assert_states_match_oracle(got, want):
    assert len(got) == len(want) and len(got) > 0
    for g, w in zip(got, want):
        assert_close(g, w, 1e-9, 1e-7)
        scale = np.abs(w["xmass1"]).max()
        assert np.abs(g["xmass1"] - w["xmass1"]).max() <= 1e-12 * scale


def assert_bitwise(ref, out, what):
    assert len(ref) == len(out)
    for i, (a, b) in enumerate(zip(ref, out)):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, "step", i, k, int((a[k] != b[k]).sum()))


def grid_tolerance(key, kind):
    conc = key in ("gridunc", "griduncn")
    if kind == "r8":
        return 1e-12 if conc else 2e-5
    return 2e-3 if conc else 5e-3


def assert_grids_close(got, want, kind, what):
    assert set(got) == set(want) and got
    for key, b in want.items():
        a = got[key].reshape(b.shape)
        err = np.abs(a - b).max() / b.max()
        print(f"[grids] {what} {kind} {key}: max |diff| / largest cell = {err:.3e} (bound {grid_tolerance(key, kind):.0e})")
        assert err <= grid_tolerance(key, kind), (what, key, err)


MATRIX = [(scn, sched) for scn in SCENARIOS for sched in SCHEDULES if sched != "as_benched" or scn in SYN_SMALL]


@pytest.mark.parametrize("scn,sched", MATRIX)
def test_fp64_schedule_matches_oracle(built, scn, sched):
    """Every schedule of the matrix, fp64, serial-stream RNG, against the oracle after every step: positions to 1e-9, velocities
    to 1e-7, no particle diverged, xmass1 to 1e-12 of its maximum.  `as_benched` (buckets 0 + time-blended wind packs: what the
    benchmark runs at 1e8 particles) also stays within 1e-11 of the unblended default run, as the blend test asks of the blend."""
    from flexpart_amd.engine import RNG_TABLE_SEQ
    n = cloud_of(scn, sched)
    got, _, rep = engine_run(scn, sched, 8, RNG_TABLE_SEQ, n)
    assert_reached(scn, sched, rep)
    want, _ = oracle_run(scn, n, "r8")
    assert_states_match_oracle(got, want)
    # the cloud is a boundary-layer cloud and stays one: the work list is what the step is about
    assert min(rep["lengths"]) > 0.3 * rep["numpart"]
    if sched == "as_benched":
        plain, _, _ = engine_run(scn, "default", 8, RNG_TABLE_SEQ, n)
        for g, p in zip(got, plain):
            for k in POS:
                assert np.abs(g[k] - p[k]).max() <= 1e-11 * max(np.abs(p[k]).max(), 1e-30), k


@pytest.mark.parametrize("mode", ["table_seq", "philox"])
@pytest.mark.parametrize("rb", [8, 4])
@pytest.mark.parametrize("scn", list(SCENARIOS))
def test_schedules_do_not_change_a_bit(built, scn, rb, mode):
    """Cost buckets, the sizes of both grids and time slices are scheduling: every array of download() after every step equals the
    default schedule's, bit for bit, in fp64 and f32, with the serial stream and the counter RNG.  (The f32 default run is the
    one the f32 parity tests hold to the r4 oracle.)"""
    from flexpart_amd.engine import RNG_PHILOX, RNG_TABLE_SEQ
    m = RNG_TABLE_SEQ if mode == "table_seq" else RNG_PHILOX
    for sched in BITWISE:
        if sched == "default":
            continue
        n = cloud_of(scn, sched)
        out, _, rep = engine_run(scn, sched, rb, m, n)
        assert_reached(scn, sched, rep)
        ref, _, ref_rep = engine_run(scn, "default", rb, m, n)      # (the golden recipes at NARROW_N particles: their own default run)
        assert ref_rep["pbl_grid"] > 1
        assert_bitwise(ref, out, (scn, sched, rb, mode))
        assert (out[-1]["ztra1"] != np.asarray(scenario(scn, n)["ztra1"])).mean() > 0.9      # the cloud did move


@pytest.mark.parametrize("kind", ["r8", "r4"])
@pytest.mark.parametrize("scn", WITH_GRIDS)
def test_grids_of_every_schedule_match_oracle(built, scn, kind):
    """gridunc / drygridunc (nest_wet: + wetgridunc and the three nested grids) of every schedule against the oracle's, at the
    tolerances of test_conccalc_and_dry_deposition_grids (float atomics sum in another order than the serial loop), and at the same
    tolerances against the default schedule's.  With buckets 0, k_pbl_finish runs in list order and the dry-deposition scatter
    (drydepo_particle<R, true>: wave_kernel_add, every lane of the wave) meets a last wave that is only partly filled: the list's
    length is not a multiple of 64."""
    from flexpart_amd.engine import RNG_TABLE_SEQ
    rb = 8 if kind == "r8" else 4
    for sched in BITWISE:
        n = cloud_of(scn, sched)
        _, og = oracle_run(scn, n, kind)
        assert og["gridunc"].sum() > 0 and og["drygridunc"].sum() > 0
        _, g, rep = engine_run(scn, sched, rb, RNG_TABLE_SEQ, n)
        if SCHEDULES[sched][0].get("pbl_cost_buckets", -1) == 0:
            assert all(length % 64 != 0 for length in rep["lengths"]), rep["lengths"]
        assert_grids_close(g, og, kind, (scn, sched, "oracle"))
        ref = engine_run(scn, "default", rb, RNG_TABLE_SEQ, n)[1]
        assert_grids_close(g, ref, kind, (scn, sched, "default"))


# ---- the ends of the work list ------------------------------------------------------------------------------------------------

EDGE_SCHEDULES = {
    "default": {},
    "buckets0": {"pbl_cost_buckets": 0},
    "default_narrow": {"pbl_grid_blocks": 1, "finish_blocks": 1},
    "buckets0_narrow": {"pbl_cost_buckets": 0, "pbl_grid_blocks": 1, "finish_blocks": 1},
}


def run_edge(sc, nsteps=2):
    """Oracle once, the four schedules of EDGE_SCHEDULES against it (fp64, serial-stream RNG) and bit for bit among themselves.
    -> the list lengths of the default run."""
    from flexpart_amd.engine import Engine, RNG_TABLE_SEQ
    from oracle.oracle import Oracle
    orc = Oracle(sc, "r8")
    orc.lib.orc_set_parallel_semantics(orc.h, 1)
    want = orc.run(nsteps)
    ref, lengths = None, None
    for name, options in EDGE_SCHEDULES.items():
        eng = Engine(sc, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_TABLE_SEQ, options=options)
        got, lens = [], []
        for _ in range(nsteps):
            eng.step()
            lens.append(eng.info("pbl_list_length"))
            got.append(eng.download())
        assert eng.counters()["n_bad_position"] == 0
        assert eng.info("pbl_grid") == 1 if "narrow" in name else eng.info("pbl_grid") > 1
        eng.close()
        assert_states_match_oracle(got, want)
        if ref is None:
            ref, lengths = got, lens
        else:
            assert_bitwise(ref, got, name)
            assert lens == lengths
    return lengths


@pytest.mark.parametrize("frac_pbl", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_work_list_edges(built, n, frac_pbl):
    """Clouds around the sizes of a wave and a block: the clamped chunk read of k_pbl_loop (min(cur + lane, nlist - 1)), its early
    return per block, `mine = i < nwork` of the list-order k_pbl_finish and the short last tile of the slot-order one.  With
    frac_pbl = 0.5 the list is shorter than the cloud and the tiles of the slot order are mixed."""
    sc = syn.small(n=n, nx=60, ny=40, nz=40, nsteps=2, ctl=5.0, ifine=4, cblflag=1, frac_pbl=frac_pbl)
    lengths = run_edge(sc)
    if frac_pbl == 1.0:
        assert lengths[0] == n      # every particle starts inside the boundary layer
    elif n >= 63:
        assert 0 < lengths[0] < n


@pytest.mark.parametrize("case", ["stable_only", "cbl_only", "neutral_only", "unstable_gaussian_only"])
def test_work_list_with_one_stability_class(built, case):
    """Every boundary-layer particle in ONE stability class (k_prep's key): three of the four class segments of the list are empty.
    stable_only is the LAST class (three empty segments ahead of it), cbl_only the first.  The class follows from the fields alone
    -- 1/L and the mixing height are the same in every column and at both times --, which is asserted on them."""
    cbl = 1 if case == "cbl_only" else 0
    sc = syn.small(n=1000, nx=60, ny=40, nz=40, nsteps=2, ctl=5.0, ifine=4, cblflag=cbl, frac_pbl=1.0, hmix_const=800.0)
    oli = {"stable_only": 0.05, "cbl_only": -0.1, "neutral_only": 1.0e-5, "unstable_gaussian_only": -0.1}[case]
    sc["oli"] = np.full_like(sc["oli"], oli)
    if case == "cbl_only":      # a convective velocity scale that goes with 1/L = -0.1 (the CBL scheme divides by powers of w*)
        sc["wstar"] = np.full_like(sc["wstar"], 1.5)
    h_over_l = sc["hmix"] * sc["oli"]
    if case == "stable_only":
        assert (h_over_l >= 1).all()                      # class 4
    elif case == "neutral_only":
        assert (np.abs(h_over_l) < 1).all()               # class 3
    elif case == "unstable_gaussian_only":
        assert (h_over_l <= -1).all() and cbl == 0        # class 2
    else:
        assert (-h_over_l > 5).all() and int(sc["cblflag"]) == 1 and int(sc["turbswitch"]) != 0      # class 1
    lengths = run_edge(sc)
    assert lengths[0] == 1000


# ---- the real grid sizes (no oracle can run there) ----------------------------------------------------------------------------

@pytest.mark.parametrize("rb", [8, 4])
def test_full_size_schedules_bitwise_and_linked_to_the_small_run(built, rb):
    """2.5e6 particles: more than 2 097 152, so the uncapped grid of k_pbl_finish (8192 blocks) is the limit and its waves walk
    several tiles / strides; more than the persistent grid of the Langevin kernel holds lanes, so its waves refill.  Counter RNG,
    global_particles = 1e8: the wind packs are blended in time as in the benchmark.
    * automatic buckets (3: slot order with the queue carry), buckets 0 (list order), buckets 0 with time slices: every array bit
      for bit, after every step;
    * 4096 consecutive particle numbers from the middle of the cloud, run alone in an engine of their own (the size and the grids
      the oracle-compared tests run), end bit for bit where they end in the big run: big-run path == small-run path == oracle;
    * no bad position; every live particle is due at every step."""
    from flexpart_amd.engine import Engine, RNG_PHILOX
    n, nsteps, lo, m = 2_500_000, 3, 1_250_000 - 2048, 4096
    assert n > 8192 * 256 and n > 262144
    sc = syn.base_scenario(60, 40, 40, ctl=5.0, ifine=4, cblflag=1, nsteps=nsteps)
    kw = dict(compute_real_bytes=rb, host_real_bytes=rb, rng_mode=RNG_PHILOX, seed=2024, global_particles=100_000_000)
    ref = first = None
    for options in ({}, {"pbl_cost_buckets": 0}, {"pbl_cost_buckets": 0, "pbl_slices": "48,96,0"}):
        eng = Engine(sc, max_particles=n, options=options, **kw)
        eng.seed_particles(n, seed=SEED, frac_pbl=0.5)
        assert eng.info("time_blended_packs") == 1
        if first is None:
            first = eng.download(lo, m)
        out = []
        alive = n
        for _ in range(nsteps):
            st = eng.step()
            assert st["n_due"] == alive and st["n_bad_position"] == 0, (options, st, alive)
            out.append(eng.download())
            # every particle that ended is in one of the step's termination counters (the CBL scheme's own blow-up, cbl.f90 has no
            # guard where its bi-Gaussian weights leave [0,1], ends a particle like one that leaves the domain); which ones end is
            # part of the bitwise comparison below
            ended = alive - int((out[-1]["itra1"] != DEAD).sum())
            assert ended == st["n_left_domain"] + st["n_min_mass"] + st["n_max_age"], (options, st, ended)
            alive -= ended
            assert eng.info("pbl_list_length") > 0.3 * n
        print(f"[full size] rb={rb} {options}: {n - alive} of {n} particles ended in {nsteps} steps")
        assert alive >= 0.999 * n      # rare events, not a leak: the cloud is still there
        assert eng.info("blended_steps") == nsteps and eng.info("pbl_grid") * 256 < n
        assert eng.info("pbl_launches_per_step") == (3 if "pbl_slices" in options else 1)
        assert eng.counters()["n_bad_position"] == 0
        eng.close()
        if ref is None:
            ref = out
        else:
            assert_bitwise(ref, out, options)
            del out
    # the slice [lo, lo + m) alone, seeded as a rank's shard of the same global cloud
    eng = Engine(sc, max_particles=m, particle_base=lo, **kw)
    eng.seed_particles(m, seed=SEED, frac_pbl=0.5)
    assert eng.info("time_blended_packs") == 1
    start = eng.download()
    assert_bitwise([first], [start], "initial state of the slice")
    part = [(eng.step(), eng.download())[1] for _ in range(nsteps)]
    eng.close()
    assert_bitwise([{k: v[..., lo:lo + m] for k, v in s.items()} for s in ref], part, "slice run alone")
    assert (part[-1]["ztra1"] != start["ztra1"]).mean() > 0.9
