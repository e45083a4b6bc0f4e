"""Per-particle averages over the output interval (ipout = 3; fpx_config.device_partavg = 1): fpx_step's k_partavg,
fpx_get_partavg, fpx_partoutput_average, fpx_partavg_time.  Reference: partpos_average.f90:31-184 (called at
timemanager.f90:617) and partoutput_average.f90:54-201 (called at timemanager.f90:455).

CPU: the numpy restatement tests/partavg_ref.py against what flang builds of the unmodified routines produce
(tests/golden/pa_r4.npz, pa_r8.npz), the coverage of the synthetic case, and -- where flang and the reference are
present -- against a fresh build.
GPU: the kernel of the step against the restatement applied to the particles downloaded after each step, and the writer
against the restatement fed the engine's own sums.

ONE RULE for every comparison.  FMA contraction is off, the divisions are IEEE and the order of operations is the
reference's on all sides, so npart_av and twelve of the fifteen arrays (z, topo, pv, qv, tt, uu, vv, rho, tro, hmix,
energy) are EQUAL.  The three Cartesian sums go through sin and cos, the two angles of a record through atan2: flang's
libm, numpy and the device's functions each lie within a few ulp of the truth and not on each other.
  * Cartesian sums after n accumulations: |diff| <= 16 n eps, eps = 2^-23 or 2^-52.  Each addend on either side is within
    3 eps of the exact value (<= 2 ulp per function on values <= 1, and one product); the n additions round by at most
    n eps / 2 |sum| <= n^2 eps / 2, with n <= 8 here.
  * The file: same length, same holes, the ten shorts that do not come from angles equal; ishort_xlon / ishort_ylat differ
    by at most 1, in at most 1 % of the written records.  The clouds lie at |lon| < 30, |lat| < 50 degrees (the special
    particles of the CPU case reach 180 and 40).
One deviation from the reference, mirrored here: a particle whose advance ended outside the grid or with a non-finite
position (nstop > 1; the step terminates it) is not averaged in that step -- the reference would index out of bounds."""
import os
import sys

import numpy as np
import pytest

import partavg_ref as pr
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ("r4", "r8")
CART = pr.SUMS[:3]


def compare_state(got, want, kind, label=""):
    """The rule above for npart_av and the fourteen sums; prints the observed maximum of the Cartesian sums in eps."""
    eps = float(np.finfo(pr.RT[kind]).eps)
    assert np.array_equal(np.asarray(got["npart_av"], np.int64), np.asarray(want["npart_av"], np.int64)), label
    for k in pr.EXACT:
        g, w = np.asarray(got[k]).astype(pr.RT[kind]), np.asarray(want[k]).astype(pr.RT[kind])
        assert np.array_equal(g, w), (label, k, int((g != w).sum()))
    n = np.maximum(np.asarray(want["npart_av"], np.float64), 1.0)
    worst = 0.0
    for k in CART:
        d = np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64))
        worst = max(worst, float((d / eps).max()))
        assert (d <= 16.0 * n * eps).all(), (label, k, float((d / (n * eps)).max()))
    print(f"{label} [{kind}] Cartesian sums: max |diff| = {worst:.2f} eps (bound 16 n eps, n <= {int(n.max())})")


def compare_file(got, want, valid, label=""):
    """The rule above for the bytes of a partposit_average file; `valid`: the restatement's mask of the written particles."""
    assert len(got) == len(want) and len(got) % 24 == 0, (label, len(got), len(want))
    g = np.frombuffer(got, "<i2").reshape(-1, 12)
    w = np.frombuffer(want, "<i2").reshape(-1, 12)
    v = np.asarray(valid)[: len(g)]
    assert len(g) == 0 or v[-1]                                   # the file ends with the last valid record
    assert not g[~v].any() and not w[~v].any(), label             # holes: zero bytes
    assert np.array_equal(g[:, 2:], w[:, 2:]), (label, np.nonzero((g[:, 2:] != w[:, 2:]).any(axis=1))[0][:5])
    d = np.abs(g[:, :2].astype(np.int64) - w[:, :2].astype(np.int64))
    nflip = int((d != 0).any(axis=1).sum())
    print(f"{label} records written {int(v.sum())}, angle shorts differing {nflip}, max difference {int(d.max()) if d.size else 0}")
    assert (d <= 1).all(), label
    assert nflip <= 0.01 * v.sum(), (label, nflip, int(v.sum()))


# ---- CPU ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated():
    """run_case() of the restatement per kind with its branch counters: computed once, never modified."""
    out = {}
    c = syn.partavg_case()
    for kind in KINDS:
        st = {}
        out[kind] = (pr.run_case(c, kind, st), st)
    return out


def gold_state(gold, iv):
    st = {k: gold[f"{k}_{iv}"] for k in pr.SUMS}
    st["npart_av"] = gold[f"npart_av_{iv}"]
    return st


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(restated, kind):
    """Both output intervals: the fifteen arrays before the output call, the file and its name, in both real kinds."""
    gold = np.load(os.path.join(GOLD, f"pa_{kind}.npz"))
    res, _ = restated[kind]
    assert len(res) == 2
    for iv, (before, rec, valid, data, name) in enumerate(res):
        ref = gold_state(gold, iv)
        assert all(ref[k].dtype == pr.RT[kind] for k in pr.SUMS)
        compare_state(before, ref, kind, f"interval {iv}")
        compare_file(data, gold[f"file_{iv}"].tobytes(), valid, f"interval {iv}")
        assert name == str(gold[f"name_{iv}"])
    assert res[0][4] == "partposit_average_20200115014500" and res[1][4] == "partposit_average_20200115023000"


@pytest.mark.parametrize("kind", KINDS)
def test_case_covers_every_branch(restated, kind):
    """Everything the two routines can do appears in the case, counted by the restatement while it runs."""
    res, st = restated[kind]
    c = syn.partavg_case()
    assert st["fixup"] > 0                                        # jyp >= nymax (partpos_average.f90:56-59)
    before, rec, valid, data, _ = res[0]
    n = int(c["npart"])
    # a particle terminated mid-interval: sums kept, no record -- a hole inside the file, and the file ends before the last ones
    gone = (before["npart_av"] == 3) & ~valid
    assert gone.any() and len(data) == 24 * (n - 3) and not rec[gone].any()
    assert gone[: n - 3].any() and valid[np.nonzero(gone)[0][0]:].any()
    assert set(np.unique(before["npart_av"][valid])) == {3, 6}    # particles with different npart_av
    # the clamps from ishort_z on: where a physical value can reach one (qv, tt, pv, energy) on at least one side
    for key in ("qv", "tt", "pv", "energy", "z", "uu", "vv"):
        assert st["clamp_hi_" + key] + st["clamp_lo_" + key] > 0, (key, st)
    assert st["clamp_hi_pv"] > 0 and st["clamp_lo_pv"] > 0
    for key in ("topo", "tro", "hmix", "rho"):                    # 2 x - 32000 of a height below 16 km, 20000 rho - 32000: out of reach
        assert st["clamp_hi_" + key] + st["clamp_lo_" + key] == 0
    # the wrap at +-180: only an 8-byte real can reach it (synthetic.partavg_case explains why)
    assert (st["wrap"] > 0) == (kind == "r8"), st
    # a second interval after the reset: the sums restart from zero
    b2 = res[1][0]
    assert set(np.unique(b2["npart_av"])) == {0, 3} and res[1][3] != res[0][3] and len(res[1][3]) == len(data)
    assert (b2["z"][b2["npart_av"] == 0] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_a_live_build_of_the_reference(kind, tmp_path):
    sys.path.insert(0, GOLD)
    import make_partavg_golden as mk
    if not mk.available():
        pytest.skip("flang or the reference tree is not present")
    exe = mk.build(kind, str(tmp_path))
    c = syn.partavg_case()
    live = mk.run(exe, c, str(tmp_path))
    mine = pr.run_case(c, kind)
    assert len(live) == len(mine) == 2
    for iv, ((st, data, name), (before, rec, valid, mydata, myname)) in enumerate(zip(live, mine)):
        compare_state(before, st, kind, f"live interval {iv}")
        compare_file(mydata, data, valid, f"live interval {iv}")
        assert name == myname


def test_header_cites_the_reference_lines():
    """The public header names the new entry points next to the reference lines they replace."""
    text = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    for name in ("fpx_get_partavg", "fpx_partoutput_average", "fpx_partavg_time", "device_partavg", "timemanager.f90:617", "timemanager.f90:455",
                 "partpos_average.f90:31-184", "partoutput_average.f90:54-201"):
        assert name in text, name


# ---- GPU ------------------------------------------------------------------------------------------------------

ENGINES = [(8, 8), (4, 4)]          # (compute_real_bytes, host_real_bytes): fp64 engine with an r8 host, f32 engine with an r4 host


def pa_scenario(nsteps=6, on=1, **kw):
    """syn.small(n=1500, nx=20, ny=12, nz=10) on a one-degree limited-area grid from (-20, 20): longitudes -20 .. -1,
    latitudes 20 .. 31; PBL and above-PBL particles; oro, pv, qv of add_partoutput_fields; every seventh particle dead."""
    sc = syn.small(n=1500, nx=20, ny=12, nz=10, nsteps=nsteps, global_grid=False, **kw)
    syn.add_partoutput_fields(sc, itime=0)
    if on:
        sc.update(ipout=3, device_partavg=1)
    z = np.asarray(sc["ztra1"])
    assert (z < sc["hmix"].min()).sum() > 100 and (z > sc["hmix"].max()).sum() > 100      # both epilogues are taken
    return sc


def kind_of(hb):
    return "r4" if hb == 4 else "r8"


def make_engine(sc, cb, hb, **kw):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    return Engine(sc, compute_real_bytes=cb, host_real_bytes=hb, rng_mode=RNG_PHILOX, seed=4711, **kw)


def averaged(sc, before, after, itime):
    """The particles the step at itime averages: due before it, and left inside the grid by advance (the deviation)."""
    nx, ny, _ = (int(v) for v in sc["grid"])
    x, y, z = after["xtra1"], after["ytra1"], after["ztra1"]
    with np.errstate(invalid="ignore"):
        inside = (x >= 0.) & (x < float(nx - 1)) & (y >= 0.) & (y <= float(ny - 1)) & np.isfinite(z)
    return (before["itra1"] == itime) & inside, (before["itra1"] == itime) & ~inside


def run_steps(eng, sc, P, nsteps, state, check_kind=None, label=""):
    """nsteps steps; the restatement follows in `state` from the downloads; with check_kind every step is compared."""
    skipped = 0
    before = eng.download()
    prev = eng.get_partavg() if check_kind else None
    for i in range(nsteps):
        itime = eng.itime
        eng.step()
        after = eng.download()
        take, skip = averaged(sc, before, after, itime)
        skipped += int(skip.sum())
        assert (after["itra1"][skip] == pr.DEAD).all()           # what is skipped is terminated in the same step
        pr.accumulate(state, P, itime, after["xtra1"], after["ytra1"], after["ztra1"], take)
        if check_kind:
            got = eng.get_partavg()
            compare_state(got, state, check_kind, f"{label} step {i}")
            for k in pr.SUMS + ("npart_av",):                     # particles not due: the engine's own values of before the step, bit for bit
                assert np.array_equal(np.asarray(got[k])[~take], np.asarray(prev[k])[~take]), (i, k)
            prev = got
        before = after
    return before, skipped


def step_parity(cb, hb, blend_mode):
    kind = kind_of(hb)
    sc = pa_scenario()
    P = pr.params_from_scenario(sc, kind)
    eng = make_engine(sc, cb, hb, blend_mode=blend_mode)
    state = pr.new_state(1500, kind)
    last, skipped = run_steps(eng, sc, P, 5, state, check_kind=kind, label=f"blend_mode {blend_mode}")
    eng.close()
    n = state["npart_av"]
    print("npart_av histogram", np.bincount(n), "particles skipped on leaving the grid", skipped)
    assert (n == 5).sum() > 1000 and (n == 0).sum() >= 1500 // 7
    assert np.count_nonzero(state["uu"]) > 1000 and np.count_nonzero(state["pv"]) > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_step_parity(built, cb, hb):
    """After each of 5 steps get_partavg equals the restatement applied to the download after that step for the particles
    due before it (the rule above); npart_av exact; particles not due unchanged.  Fails on an engine without the feature:
    it refuses the configuration."""
    step_parity(cb, hb, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_step_parity_with_the_blended_wind_pack(built, cb, hb):
    """blend_mode = 1: the step gathers its winds from the blended pack, the averages still read the two unblended slots --
    the uu / vv sums are exact against the restatement, which interpolates per slot and then in time."""
    step_parity(cb, hb, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_the_feature_changes_nothing_else(built, cb, hb):
    """Particle arrays and gridunc after 3 steps are bitwise the same with the option on (ipout = 3) and off (ipout = 0).
    As in test_calcfluxes.py the sampling puts each particle's whole dyadic mass into its own cell (lusekerneloutput = 0,
    ind_samp = 0), so every sum of gridunc is exact in any order of the atomics."""
    res = []
    for on in (1, 0):
        sc = pa_scenario(on=on)
        dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
        syn.add_outgrid(sc, 12, 8, 3, dxout=dx / 2.0, dyout=dy / 2.0, outlon0=xlon0 + 6.0 * dx, outlat0=ylat0 + 3.0 * dy, old_fraction=0.0)
        h = syn._splitmix64(1500, 0xF1)
        sc["xmass1"] = np.stack([(1 + (h % np.uint64(8)).astype(np.int64)).astype(np.float64) / 1024.0])
        sc["lusekerneloutput"] = 0
        sc["concflags"] = np.array([0, int(sc["concflags"][1])], np.int32)
        eng = make_engine(sc, cb, hb)
        for _ in range(3):
            eng.step()
            eng.conccalc(eng.itime, 1.0)
        res.append((eng.download(), eng.grids()[0]))
        eng.close()
    (a, ga), (b, gb) = res
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    print("gridunc cells set", np.count_nonzero(ga), "differing", np.count_nonzero(ga != gb))
    assert np.array_equal(ga, gb) and ga.sum() > 0


def expected_file(eng, kind, itime):
    """The restatement's writer fed the engine's own sums and itra1: (bytes, validity mask, number of records)."""
    st = eng.get_partavg()
    itra1 = eng.download()["itra1"]
    rec, valid = pr.records(st, itra1, itime, kind)
    return pr.file_bytes(rec, valid), valid


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_the_file(built, tmp_path, cb, hb):
    """After 4 steps: name, length, holes and records of partoutput_average against the restatement fed the engine's own
    downloaded sums; all fifteen arrays zero afterwards; a second interval gives a second, correct file; nrecords."""
    kind = kind_of(hb)
    sc = pa_scenario()
    eng = make_engine(sc, cb, hb)
    prefix = str(tmp_path) + os.sep
    names = []
    for iv, nsteps in enumerate((4, 2)):
        for _ in range(nsteps):
            eng.step()
        want, valid = expected_file(eng, kind, eng.itime)
        name, nrec = eng.partoutput_average(eng.itime, prefix, bdate=syn.GV_BDATE)
        assert os.path.basename(name) == pr.file_name(syn.GV_BDATE, eng.itime)
        compare_file(open(name, "rb").read(), want, valid, f"interval {iv}")
        assert nrec == int(valid.sum()) and nrec > 1000
        assert (~valid[: len(want) // 24]).sum() > 100            # holes inside the file (every seventh particle is dead)
        after = eng.get_partavg()
        assert all(not np.asarray(after[k]).any() for k in after)
        names.append(name)
    eng.close()
    assert names[0] != names[1] and os.path.basename(names[0]) == "partposit_average_20200115010000"


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_sort_in_the_middle_of_an_interval(built, tmp_path, cb, hb):
    """fpx_sort_particles after two of four steps changes neither get_partavg nor the file, bitwise."""
    sc = pa_scenario()
    res = []
    for sort in (False, True):
        eng = make_engine(sc, cb, hb)
        for i in range(4):
            if sort and i == 2:
                eng.sort()
            eng.step()
        st = eng.get_partavg()
        path = str(tmp_path / f"pa_{int(sort)}")
        eng.partoutput_average(eng.itime, path)
        res.append((st, open(path, "rb").read()))
        eng.close()
    (a, fa), (b, fb) = res
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert fa == fb and len(fa) > 24 * 1000 and (a["npart_av"] == 4).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_checkpoint_carries_the_sums(built, tmp_path, cb, hb):
    """Written after two of four steps and read into a fresh engine that finishes the interval: the file is byte-identical
    to the uninterrupted run's.  A checkpoint read with a mismatched option is refused, both ways."""
    sc = pa_scenario()
    eng = make_engine(sc, cb, hb)
    for _ in range(2):
        eng.step()
    ck = str(tmp_path / "ck.bin")
    eng.checkpoint_write(ck)
    for _ in range(2):
        eng.step()
    itime = eng.itime
    eng.partoutput_average(itime, str(tmp_path / "whole"))
    eng.close()
    eng = make_engine(sc, cb, hb)
    eng.checkpoint_read(ck)
    mid = eng.get_partavg()
    assert (mid["npart_av"] == 2).sum() > 1000
    for _ in range(2):
        eng.step()
    assert eng.itime == itime
    eng.partoutput_average(itime, str(tmp_path / "resumed"))
    eng.close()
    whole, resumed = (tmp_path / "whole").read_bytes(), (tmp_path / "resumed").read_bytes()
    assert whole == resumed and len(whole) > 24 * 1000
    off = pa_scenario(on=0)
    eng = make_engine(off, cb, hb)
    with pytest.raises(Exception, match="device_partavg"):
        eng.checkpoint_read(ck)
    for _ in range(2):
        eng.step()
    plain = str(tmp_path / "plain.bin")
    eng.checkpoint_write(plain)
    eng.close()
    eng = make_engine(sc, cb, hb)
    with pytest.raises(Exception, match="device_partavg"):
        eng.checkpoint_read(plain)
    eng.close()
    assert os.path.getsize(ck) - os.path.getsize(plain) == 8 + 1500 * (4 + 14 * hb)
    for file, flag in ((plain, 0), (ck, 2)):
        assert np.frombuffer(open(file, "rb").read(64)[60:64], np.int32)[0] == flag


@pytest.mark.gpu
def test_states_and_refusals(built):
    from flexpart_amd.engine import Engine, _vp
    sc = syn.small(n=10, nx=20, ny=12, nz=10, nsteps=1, global_grid=False)
    sc["ipout"] = 3
    with pytest.raises(Exception, match="ipout = 3: the particle loop's partpos_average .timemanager.f90:617. is not computed by this engine") as e:
        Engine(sc)                                           # ipout = 3 alone: refused as before, same status, same text
    assert e.value.code == -5                                # FPX_ERR_UNSUPPORTED
    sc["device_partavg"] = 2
    with pytest.raises(Exception, match="device_partavg must be 0 or 1") as e:
        Engine(sc)
    assert e.value.code == -1                                # FPX_ERR_ARG
    sc["device_partavg"] = 1
    eng = Engine(sc)                                         # accepted; the scenario has no oro / pv / qv: no diag fields on the device
    with pytest.raises(Exception, match="device_partavg = 1 needs oro, pv, qv, tt of both slots") as e:
        eng.step()
    assert e.value.code == -3                                # FPX_ERR_STATE
    eng.close()
    sc["ipout"] = 0
    with pytest.raises(Exception, match="device_partavg = 1 without ipout = 3") as e:
        Engine(sc)
    assert e.value.code == -1                                # FPX_ERR_ARG
    sc["device_partavg"] = 0
    eng = Engine(sc)                                         # an engine without the option: no sums to fetch, no file to write
    n = np.zeros(10, np.int32)
    assert eng.lib.fpx_get_partavg(eng.h, 0, 10, _vp(n), None) == -3
    assert b"created without device_partavg" in eng.lib.fpx_last_error()
    assert eng.lib.fpx_partoutput_average(eng.h, 0, b"/nonexistent/x", None) == -3
    assert b"created without device_partavg" in eng.lib.fpx_last_error()
    eng.close()


@pytest.mark.gpu
def test_kernel_time(built):
    """fpx_partavg_time: one launch per step and a positive device time; reset starts over."""
    eng = make_engine(pa_scenario(), 8, 8)
    for _ in range(3):
        eng.step()
    ms, launches = eng.partavg_time(reset=True)
    assert launches == 3 and ms > 0
    eng.step()
    ms, launches = eng.partavg_time()
    eng.close()
    assert launches == 1 and ms > 0
