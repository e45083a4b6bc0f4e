"""Gross mass fluxes (calcfluxes.f90, fluxoutput.f90; fpx_config.device_flux = 1).

CPU: the numpy restatement tests/calcfluxes_ref.py against what flang builds of the unmodified routines produce
(tests/golden/cf_r4.npz, cf_r8.npz: the flux array bit for bit, the grid_flux file byte for byte), the coverage of the
synthetic case, and -- where flang and the reference are present -- against a fresh build.
GPU: the two kernels of the step against the restatement applied to the particles downloaded before and after each step.
FMA contraction is off and the divisions are IEEE on both sides and the masses are dyadic, so every comparison is exact:
there is nothing for a tolerance to absorb."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import calcfluxes_ref as cr
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ("r4", "r8")


# ---- CPU ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated():
    """(flux, stats) of the restatement per (kind, variant): computed once, never modified."""
    out = {}
    for kind in KINDS:
        for v in syn.CF_VARIANTS:
            st = {}
            flux = cr.run_case(syn.calcfluxes_case(v), kind, st)
            flux.setflags(write=False)
            out[kind, v] = (flux, st)
    return out


@pytest.mark.parametrize("variant", syn.CF_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(restated, kind, variant):
    """flux after all calls bit for bit, the file of fluxoutput byte for byte and its name, in both real kinds."""
    gold = np.load(os.path.join(GOLD, f"cf_{kind}.npz"))
    c = syn.calcfluxes_case(variant)
    flux, _ = restated[kind, variant]
    ref = gold[f"flux_{variant}"]
    assert flux.dtype == ref.dtype == cr.RT[kind] and flux.shape == ref.shape
    assert np.array_equal(flux, ref)
    assert np.count_nonzero(ref) > 50
    data = cr.fluxoutput(flux, kind, c["itime"], c["area"], c["areaeast"], c["areanorth"], c["outstep"])
    assert data == gold[f"file_{variant}"].tobytes()
    assert cr.flux_file_name(c["bdate"], c["itime"], kind) == str(gold[f"name_{variant}"]) == "grid_flux_20200115030000"


@pytest.mark.parametrize("kind", KINDS)
def test_case_covers_every_branch(restated, kind):
    """Everything the routine can do appears in the 'release' case, counted by the restatement while it runs."""
    flux, st = restated[kind, "release"]
    for key in ("east_one", "east_many", "west_one", "west_many", "north_one", "north_many", "south_one", "south_many",
                "up_one", "up_many", "down_one", "down_many",                 # faces: one and several, all six directions
                "above_top",                                                  # kzave = numzgrid + 1: no horizontal flux
                "trunc_west", "trunc_south",                                  # int() of a mean less than a cell outside -> cell 0
                "face_x_below", "face_x_above", "face_y_below", "face_y_above",   # face indices outside the grid, each side
                "cyclic_eastward", "cyclic_westward",                        # |xold - xtra1| >= nx/2, both directions
                "age1", "age2", "kp_gt_1"):
        assert st[key] > 0, (key, st)
    assert st["cyclic_added"] == 0         # ixs of calcfluxes.f90:122 is far below 0 on any sane grid: the branch adds nothing
    assert st["guarded"] == 0              # no particle of the fixtures needs the engine's guards
    assert all(np.count_nonzero(flux[..., i]) > 0 for i in range(6))
    assert np.count_nonzero(flux[:, 1:]) > 0 and np.count_nonzero(flux[1]) > 0
    sparse, full = cr.file_formats(flux)                                      # [nage][nspec][6]
    assert sparse.any(axis=2).all() and full.any(axis=2).all()                # per (species, age class): both formats
    # mdomainfill = 1: kp = 1 although npoint is the particle number
    fl2, st2 = restated[kind, "domainfill"]
    assert st2["kp_gt_1"] == 0 and np.count_nonzero(fl2[:, 1:]) == 0 and np.count_nonzero(fl2[:, 0]) > 0
    assert int(syn.calcfluxes_case("domainfill")["npoint0"].max()) > 3


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_a_live_build_of_the_reference(kind, tmp_path):
    sys.path.insert(0, GOLD)
    import make_calcfluxes_golden as mk
    if not mk.available():
        pytest.skip("flang or the reference tree is not present")
    exe = mk.build(kind, str(tmp_path))
    for v in syn.CF_VARIANTS:
        c = syn.calcfluxes_case(v)
        flux, data, name = mk.run(exe, c, str(tmp_path))
        mine = cr.run_case(c, kind)
        assert np.array_equal(mine.astype(np.float64), flux), v
        assert cr.fluxoutput(mine, kind, c["itime"], c["area"], c["areaeast"], c["areanorth"], c["outstep"]) == data, v
        assert cr.flux_file_name(c["bdate"], c["itime"], kind) == name


def test_header_cites_the_reference_lines():
    """The public header names the new entry points next to the reference lines they replace."""
    text = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    for name in ("fpx_get_flux", "fpx_fluxoutput", "fpx_calcfluxes_time", "device_flux", "timemanager.f90:623", "timemanager.f90:439",
                 "fluxoutput.f90:46-283", "calcfluxes.f90:43-166"):
        assert name in text, name


# ---- GPU ------------------------------------------------------------------------------------------------------

ENGINES = [(8, 8), (4, 4)]          # (compute_real_bytes, host_real_bytes): fp64 engine with an r8 host, f32 engine with an r4 host


def flux_scenario(nspec=1, outgrid=(12, 8, 3), nsteps=3, device_flux=1, points=False, **kw):
    """syn.small(n=1500, nx=20, ny=12, nz=10) on a one-degree grid, the cloud drawn together over six by four met cells
    around an output grid of quarter cells, PBL and above-PBL particles, dyadic masses.  points: three release points with
    ioutputforeachrelease = 1 and two age classes (particles up to 3000 s old, lage = 1800, ...)."""
    sc = syn.small(n=1500, nx=20, ny=12, nz=10, nsteps=nsteps, nspec=nspec, global_grid=False, **kw)
    nx, ny = 20, 12
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    sc["xtra1"] = 6.0 + 6.0 * np.asarray(sc["xtra1"]) / float(nx - 1)
    sc["ytra1"] = 3.0 + 4.0 * np.asarray(sc["ytra1"]) / float(ny - 1)
    nxg, nyg, nzg = outgrid
    syn.add_outgrid(sc, nxg, nyg, nzg, dxout=dx / 4.0, dyout=dy / 4.0, outlon0=xlon0 + 7.5 * dx, outlat0=ylat0 + 4.0 * dy, old_fraction=0.0)
    if points:
        syn.add_release_points(sc, xmass=[[1.0, 1.0, 1.0]] * nspec, npart_rel=[500, 500, 500], lage=[1800, 999999999], max_age=3000)
    h = syn._splitmix64(1500, 0xF1)
    sc["xmass1"] = np.stack([(1 + ((h >> np.uint64(8 * k)) % np.uint64(8)).astype(np.int64)).astype(np.float64) / 1024.0 for k in range(nspec)])
    if device_flux:
        sc.update(iflux=1, device_flux=1)
    z = np.asarray(sc["ztra1"])
    assert (z < sc["hmix"].min()).sum() > 100 and (z > sc["hmix"].max()).sum() > 100      # both epilogues are taken
    return sc


def kind_of(hb):
    return "r4" if hb == 4 else "r8"


def make_engine(sc, cb, hb, **kw):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    return Engine(sc, compute_real_bytes=cb, host_real_bytes=hb, rng_mode=RNG_PHILOX, seed=4711, **kw)


def expected(P, itime, before, after, flux=None, masses=None):
    """The restatement applied to two downloads around a step at `itime`."""
    flux = P.new_flux() if flux is None else flux
    due = before["itra1"] == itime
    m = (before["xmass1"] if masses is None else masses)[:, due]
    return cr.calcfluxes(flux, P, itime, before["xtra1"][due], before["ytra1"][due], before["ztra1"][due],
                         after["xtra1"][due], after["ytra1"][due], after["ztra1"][due], m, before["npoint"][due], before["itramem"][due])


def stepped(eng, P, nsteps, clear):
    """nsteps steps: per step the fetched flux (clear: fetched with clear after every step) and the restatement's."""
    got, want, downloads = [], [], [eng.download()]
    acc = P.new_flux()
    for _ in range(nsteps):
        itime = eng.itime
        eng.step()
        downloads.append(eng.download())
        if clear:
            want.append(expected(P, itime, downloads[-2], downloads[-1]))
            got.append(eng.get_flux(clear=True))
        else:
            expected(P, itime, downloads[-2], downloads[-1], flux=acc)
    if not clear:
        got.append(eng.get_flux()); want.append(acc)
    return got, want, downloads


@pytest.mark.gpu
@pytest.mark.parametrize("points", [False, True])
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_step_parity(built, cb, hb, points):
    """flux after each of 3 steps (fetched with clear) and accumulated over all three equals the restatement applied to
    the downloads, exactly, zero cells included.  Fails on an engine without the feature: it refuses the configuration."""
    sc = flux_scenario(points=points)
    P = cr.params_from_scenario(sc, kind_of(hb))
    eng = make_engine(sc, cb, hb)
    got, want, _ = stepped(eng, P, 3, clear=True)
    eng.close()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape
        print(f"step {i}: cells set {np.count_nonzero(w)}, differing {np.count_nonzero(g != w)}, per direction {[int(np.count_nonzero(w[..., d])) for d in range(6)]}")
        assert np.array_equal(g, w), i
    total = sum(np.count_nonzero(w[..., :4]) for w in want)
    assert total > 20 and sum(np.count_nonzero(w[..., 4:]) for w in want) > 5      # horizontal and vertical crossings did occur
    eng = make_engine(sc, cb, hb)
    got, want, _ = stepped(eng, P, 3, clear=False)
    ms, launches = eng.calcfluxes_time()
    eng.close()
    assert np.array_equal(got[0], want[0]) and np.count_nonzero(want[0]) > 25
    assert launches == 3 and ms > 0
    if points:
        assert want[0].shape[:2] == (2, 3) and all(np.count_nonzero(want[0][a, k]) > 0 for a in range(2) for k in range(3))


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_the_feature_changes_nothing_else(built, cb, hb):
    """Particle arrays and gridunc after 3 steps are bitwise the same with device_flux on and off.  gridunc is summed with
    atomics in an order that differs from run to run, so the sampling puts each particle's whole (dyadic) mass into its own
    cell (lusekerneloutput = 0, and ind_samp = 0: no division by the air density, conccalc.f90:80-122): every sum is then
    exact in any order and 'bitwise' is a property of the engine, not of the scheduler.  (With the 4-cell kernel two runs of the SAME configuration differ in the last bits.)"""
    res = []
    for on in (1, 0):
        sc = flux_scenario(device_flux=on)
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
    print("gridunc cells set", np.count_nonzero(ga), "differing", np.count_nonzero(ga != gb), "max |diff|", np.abs(ga - gb).max())
    assert np.array_equal(ga, gb) and ga.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_pre_epilogue_mass(built, cb, hb):
    """One step with decay and dry deposition: the flux carries the masses as they were before the step's epilogue
    (timemanager.f90:623 comes before :637-660), not the ones after it."""
    sc = flux_scenario()
    sc.update(drydep=1, drydepspec=np.array([1], np.int32), decay=np.array([2.0e-5]))
    P = cr.params_from_scenario(sc, kind_of(hb))
    eng = make_engine(sc, cb, hb)
    before = eng.download()
    itime = eng.itime
    eng.step()
    after = eng.download()
    got = eng.get_flux()
    eng.close()
    assert np.any(after["xmass1"] < before["xmass1"])
    assert np.array_equal(got, expected(P, itime, before, after))
    assert not np.array_equal(got, expected(P, itime, before, after, masses=after["xmass1"]))


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_order_against_the_receptor_block(built, cb, hb):
    """Backward run with DRYBKDEP, two species, the second without DRYDEPSPEC: the receptor block zeroes its mass before
    the particle is moved (timemanager.f90:578), and calcfluxes sees that -- its flux is exactly zero everywhere."""
    sc = flux_scenario(nspec=2, ldirect=-1)
    sc.update(drydep=1, drydepspec=np.array([1, 0], np.int32), xmass=np.array([1.0, 2.0]), drybkdep=1,
              zpoint1=np.array([0.0]), zpoint2=np.array([30.0]))
    P = cr.params_from_scenario(sc, kind_of(hb))
    eng = make_engine(sc, cb, hb)
    before = eng.download()
    itime = eng.itime
    eng.step()
    after = eng.download()
    got = eng.get_flux()
    eng.close()
    assert np.count_nonzero(got[:, :, 1]) == 0 and np.count_nonzero(got[:, :, 0]) > 10
    masses = before["xmass1"].copy()
    masses[1] = 0.0
    assert np.array_equal(got, expected(P, itime, before, after, masses=masses))


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_resort_gives_the_same_flux(built, cb, hb):
    sc = flux_scenario()
    res = []
    for si in (0, 1):
        eng = make_engine(sc, cb, hb, sort_interval=si)
        for _ in range(3):
            eng.step()
        res.append(eng.get_flux())
        eng.close()
    assert np.array_equal(res[0], res[1]) and np.count_nonzero(res[0]) > 25


@pytest.mark.gpu
def test_states_and_refusals(built):
    from flexpart_amd.engine import Engine
    sc = syn.small(n=10, nx=20, ny=12, nz=10, nsteps=1)
    sc["iflux"] = 1
    with pytest.raises(Exception, match="iflux = 1: the particle loop's calcfluxes .timemanager.f90:623. is not computed by this engine") as e:
        Engine(sc)                                           # iflux = 1 alone: refused as before, same status, same text
    assert e.value.code == -5                                # FPX_ERR_UNSUPPORTED
    sc["device_flux"] = 1
    eng = Engine(sc)                                         # accepted; no output grid yet
    with pytest.raises(Exception, match="fpx_outgrid_init"):
        eng.step()                                           # FPX_ERR_STATE: a step with device_flux on and no output grid
    out = np.zeros(16, np.float64)
    from flexpart_amd.engine import _vp
    assert eng.lib.fpx_get_flux(eng.h, _vp(out), 0, 0) == -3      # FPX_ERR_STATE: fpx_get_flux before fpx_outgrid_init
    eng.close()
    sc["iflux"] = 0
    with pytest.raises(Exception, match="device_flux = 1 without iflux = 1") as e:
        Engine(sc)
    assert e.value.code == -1                                # FPX_ERR_ARG
    sc["device_flux"] = 0
    eng = Engine(sc)
    assert eng.lib.fpx_get_flux(eng.h, _vp(out), 0, 0) == -3      # an engine without the feature has no flux to fetch
    eng.close()


def _areas(sc, seed):
    nxg, nyg, nzg = (int(v) for v in sc["outgrid"])
    return (1.0e8 * (1.0 + np.floor(syn._hash01((nyg, nxg), seed) * 64.0) / 64.0),
            1.0e6 * (1.0 + np.floor(syn._hash01((nzg, nyg, nxg), seed + 1) * 64.0) / 64.0),
            1.0e6 * (1.0 + np.floor(syn._hash01((nzg, nyg, nxg), seed + 2) * 64.0) / 64.0))


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_fluxoutput_file(built, tmp_path, cb, hb):
    """fpx_fluxoutput from the device grid = the restatement's writer fed the fetched grid, byte for byte, on a 6 x 4 x 2
    grid where both formats occur; the grid is zero afterwards."""
    kind = kind_of(hb)
    sc = flux_scenario(outgrid=(6, 4, 2))
    eng = make_engine(sc, cb, hb)
    for _ in range(3):
        eng.step()
    flux = eng.get_flux()
    area, ae, an = _areas(sc, 8500)
    prefix = str(tmp_path) + os.sep
    name = eng.fluxoutput(eng.itime, prefix, area, ae, an, outstep=3600.0, bdate=syn.GV_BDATE)
    after = eng.get_flux()
    eng.close()
    sparse, full = cr.file_formats(flux)
    assert sparse.any() and full.any()
    assert os.path.basename(name) == cr.flux_file_name(syn.GV_BDATE, 2700, kind)
    assert open(name, "rb").read() == cr.fluxoutput(flux, kind, 2700, area, ae, an, 3600.0)
    assert np.count_nonzero(after) == 0 and np.count_nonzero(flux) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", ENGINES)
def test_checkpoint_carries_the_flux(built, tmp_path, cb, hb):
    """Written after step 2 and restored into a fresh engine, step 3 leaves flux and particles bitwise the uninterrupted
    run's; a file of one kind is refused by an engine of the other; without the feature the file has the length it always had."""
    sc = flux_scenario()
    eng = make_engine(sc, cb, hb)
    for _ in range(2):
        eng.step()
    path = str(tmp_path / "ck.bin")
    eng.checkpoint_write(path)
    eng.step()
    want_flux, want_p = eng.get_flux(), eng.download()
    eng.close()
    eng = make_engine(sc, cb, hb)
    eng.checkpoint_read(path)
    eng.step()
    got_flux, got_p = eng.get_flux(), eng.download()
    eng.close()
    assert np.array_equal(got_flux, want_flux) and np.count_nonzero(want_flux) > 25
    for k in want_p:
        assert np.array_equal(got_p[k], want_p[k]), k
    # the other kind of engine refuses the file, both ways, and keeps its state
    off = flux_scenario(device_flux=0)
    eng = make_engine(off, cb, hb)
    p0 = eng.download()
    with pytest.raises(Exception, match="device_flux"):
        eng.checkpoint_read(path)
    p1 = eng.download()
    assert all(np.array_equal(p0[k], p1[k]) for k in p0)
    for _ in range(2):
        eng.step()
    plain = str(tmp_path / "plain.bin")
    eng.checkpoint_write(plain)
    eng.close()
    eng = make_engine(sc, cb, hb)
    with pytest.raises(Exception, match="device_flux"):
        eng.checkpoint_read(plain)
    eng.close()
    # length: the flux section is a count and the values, flagged in the header's reserved word; without it the file is the
    # one written before the feature existed: header, RNG state, particle arrays, grids (no receptors, no convection here)
    n_flux = want_flux.size
    assert os.path.getsize(path) - os.path.getsize(plain) == 8 + n_flux * hb
    for file, flag in ((plain, 0), (path, 1)):
        raw = open(file, "rb").read(192)
        assert np.frombuffer(raw[60:64], np.int32)[0] == flag
        numpart = int(np.frombuffer(raw[24:32], np.int64)[0])
        g3, g2, g3n, g2n, nrec, rng_bytes, cbase = (int(v) for v in np.frombuffer(raw[64:120], np.uint64))
        assert (numpart, g3n, g2n, nrec, cbase) == (1500, 0, 0, 0, 0) and g3 == 12 * 8 * 3 and g2 == 12 * 8
        per_particle = 2 * 8 + 7 * cb + 6 * 4 + 2 + cb
        base = 192 + rng_bytes + numpart * per_particle + g3 * cb + 2 * g2 * 4
        assert int(np.frombuffer(raw[184:192], np.uint64)[0]) == os.path.getsize(file) == base + flag * (8 + n_flux * hb)


WORKER = textwrap.dedent("""
    import os, sys
    sys.path[:0] = [%(root)r, %(tests)r]
    import numpy as np
    from flexpart_amd import sharding
    import test_calcfluxes as t
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    sc = t.flux_scenario()
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
        sc = sharding.shard_scenario(sc, world, rank)
    eng = t.make_engine(sc, 8, 8)
    if world > 1:
        eng.comm_init_host(dist, world, rank)
    for _ in range(3):
        eng.step()
    red = eng.get_flux(allreduce=world > 1)
    own = eng.get_flux()
    np.savez(%(out)r + f"_{world}_{rank}.npz", red=red, own=own)
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
""")


@pytest.mark.gpu
def test_two_ranks_one_gpu(built, tmp_path):
    """Two processes share the cloud and one GPU and reduce through the host transport (as tests/test_multirank_gpu.py
    does): the reduced flux is the single rank's, exactly, and the ranks' partial sums stay."""
    out = str(tmp_path / "fx")
    port = 37500 + (os.getpid() % 2000)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    ws = tmp_path / "worker.py"
    ws.write_text(WORKER % dict(root=ROOT, tests=HERE, port=port, out=out))
    procs = [subprocess.Popen([sys.executable, str(ws), str(r), "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    r = subprocess.run([sys.executable, str(ws), "0", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    a, b, s = (np.load(out + f"_{w}_{k}.npz") for w, k in ((2, 0), (2, 1), (1, 0)))
    assert np.array_equal(a["red"], s["own"]) and np.array_equal(b["red"], s["own"]) and np.count_nonzero(s["own"]) > 25
    assert np.array_equal(a["own"] + b["own"], s["own"])
    assert np.count_nonzero(a["own"]) > 0 and np.count_nonzero(b["own"]) > 0 and not np.array_equal(a["own"], a["red"])
