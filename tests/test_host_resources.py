"""The host side of the engine around its kernels: the per-step timers (fpx_kernel_time(s), fpx_calcfluxes_time,
fpx_partavg_time), the scratch buffers that grow with the particle count, and the one-shot timings of the field
preparation (fpx_verttransform_time, fpx_calcpv_time, fpx_calcpar_time, fpx_getvdep_time).  What these tests pin is
behaviour a change of the engine's buffer and event bookkeeping must not move; they need nothing but the C ABI."""
import numpy as np
import pytest

from flexpart_amd import synthetic as syn

NX, NY, NZ = 40, 24, 30


@pytest.mark.gpu
def test_timers_fold_across_the_pool_limit(built):
    """70 steps without a read: every timer folds its waiting event sets into its totals at 64 and still counts each
    step once.  The step's total and its first three parts are sums of the same event stamps."""
    from flexpart_amd.engine import Engine, RNG_PHILOX
    sc = syn.small(n=2000, nx=NX, ny=NY, nz=NZ, nsteps=70)
    syn.add_partoutput_fields(sc, itime=0)
    dx, dy, xlon0, ylat0 = (float(v) for v in sc["geom"])
    syn.add_outgrid(sc, 12, 8, 3, dxout=dx, dyout=dy, outlon0=xlon0 + 10.0 * dx, outlat0=ylat0 + 6.0 * dy, old_fraction=0.0)
    sc.update(iflux=1, device_flux=1, ipout=3, device_partavg=1)
    sc["memtime"] = np.array([0, 72 * 900], np.int32)          # the wind-time window holds all 70 steps
    eng = Engine(sc, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_PHILOX, seed=4711)
    for _ in range(70):
        eng.step()
    parts, n_parts = eng.kernel_times()
    total, n_total = eng.kernel_time()
    fx_ms, n_fx = eng.calcfluxes_time()
    pa_ms, n_pa = eng.partavg_time()
    print(f"70 steps: step {total:.3f} ms, parts {parts}, calcfluxes {fx_ms:.3f} ms, partavg {pa_ms:.3f} ms")
    assert (n_parts, n_total, n_fx, n_pa) == (70, 70, 70, 70)
    assert total > 0 and fx_ms > 0 and pa_ms > 0 and all(p > 0 for p in parts)
    assert abs(total - sum(parts[:3])) <= 1e-4 * total
    eng.kernel_times(reset=True); eng.calcfluxes_time(reset=True); eng.partavg_time(reset=True)
    for _ in range(3):
        eng.step()
    assert eng.kernel_times()[1] == 3 and eng.kernel_time()[1] == 3
    assert eng.calcfluxes_time()[1] == 3 and eng.partavg_time()[1] == 3
    eng.close()


# ---- growth ----------------------------------------------------------------------------------------------------

CAP, LIVE = 4096, 4000
STATE = ("xtra1", "ytra1", "ztra1", "uap", "ucp", "uzp", "us", "vs", "ws", "itra1", "itramem", "idt", "npoint", "nclass",
         "itrasplit", "cbt", "xmass1")


def cloud():
    """The scenario with every particle array the engine keeps, for all CAP storage spaces: LIVE particles (every seventh
    terminated) and a terminated tail, so that an upload defines the whole state whatever the engine held before."""
    sc = syn.small(n=CAP, nx=NX, ny=NY, nz=NZ, nsteps=1)
    syn.add_partoutput_fields(sc, itime=0)
    sc["itra1"][LIVE:] = -999999999
    zr, zi = np.zeros(CAP), np.zeros(CAP, np.int32)
    sc.update(uap=zr, ucp=zr, uzp=zr, us=zr, vs=zr, ws=zr, idt=zi, cbt=np.zeros(CAP, np.int16), itrasplit=np.full(CAP, 999999999, np.int32))
    return sc


def first(sc, n):
    """The same scenario with the first n particles only."""
    out = dict(sc, npart=n)
    for k in STATE:
        out[k] = np.asarray(sc[k])[..., :n]
    return out


def release_tables(kind="r8"):
    """Five small release points on this grid (synthetic.release_case): at most 96 particles over the run."""
    from oracle.oracle import rl_juldate
    rs = syn.release_case(NX, NY, NZ, nspec=1, existing=0, maxpart=CAP)
    rs["npart_rel"] = np.array([16, 24, 16, 24, 16], np.int32)
    return dict(rs, bdate_jul=rl_juldate(int(rs["bdate"][0]), int(rs["bdate"][1]), kind))


def calls(eng, sc, n, path):
    """Load n particles of sc, then step, sort, partoutput, releaseparticles; what they leave behind."""
    eng.upload_particles_from_scenario(first(sc, n))
    eng.set_numpart(min(n, LIVE))
    eng.itime = 0
    eng.step()
    eng.sort()
    nrec = eng.partoutput(eng.itime, path)
    nrel = eng.releaseparticles(eng.itime)
    return dict(download=eng.download(), file=open(path, "rb").read(), nrec=nrec, nrel=nrel, n=eng.n)


def grown(sc, rs, n_first, tmp_path, tag):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    eng = Engine(first(sc, n_first), compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_PHILOX, seed=4711, max_particles=CAP)
    eng.upload_diag_fields_from_scenario(sc)
    eng.release_init(rs)
    eng.set_option("permute", "staged")
    a = calls(eng, sc, n_first, str(tmp_path / f"{tag}_1"))
    b = calls(eng, sc, CAP, str(tmp_path / f"{tag}_2"))
    eng.close()
    return a, b


@pytest.mark.gpu
def test_scratch_growth_changes_no_result(built, tmp_path):
    """One engine of capacity 4096 makes its calls at 300 particles, then at 4000: every scratch buffer grows between the
    two rounds.  A second engine makes both rounds at 4000 and never grows.  With the counter generator (keyed on the
    particle number, the step count and the release count, which agree) the second rounds are bitwise equal."""
    sc, rs = cloud(), release_tables()
    small_first, grew = grown(sc, rs, 300, tmp_path, "grow")
    _, flat = grown(sc, rs, CAP, tmp_path, "flat")
    assert small_first["n"] < 400 and small_first["nrec"] > 200 and small_first["nrel"] > 0
    assert grew["nrec"] > 3000 and grew["nrel"] > 0 and grew["n"] >= LIVE
    assert (grew["nrec"], grew["nrel"], grew["n"]) == (flat["nrec"], flat["nrel"], flat["n"])
    for k in grew["download"]:
        assert np.array_equal(grew["download"][k], flat["download"][k]), k
    assert grew["file"] == flat["file"] and len(grew["file"]) > 3000 * 50


# ---- one-shot timings ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_repeated_one_shot_timings(built):
    """verttransform with the PV computed on the device, calcpar and getvdep, twice on one engine: each call reports a
    positive device time of its own and the second call's outputs equal the first's."""
    import test_getvdep as tg
    from flexpart_amd.engine import Engine
    nspec = 2
    ms, cins, gins = tg.chain_inputs(NX, NY, NZ)
    m, cin, gin = ms[0], cins[0], gins[0]
    eng = Engine(tg.scenario(NX, NY, NZ, nspec, m["geom"], skip=("height", "nmixz")), compute_real_bytes=8, host_real_bytes=8)
    eng.getvdep_init(syn.getvdep_tables(NX, NY, nspec))
    res = []
    for i in range(2):
        vt = eng.verttransform(1, m, None, init=(i == 0), want=("uu", "ww", "tt", "pv", "rho"), device_pv=True)
        cp = eng.calcpar(1, cin, device_vdep=True)
        gv = eng.getvdep(1, gin)
        print(f"call {i}: vt {vt['device_ms']:.4f} ms, pv {vt['calcpv_ms']:.4f} ms, cp {cp['device_ms']:.4f} ms, gv {gv['device_ms']:.4f} ms")
        assert vt["device_ms"] > 0 and vt["calcpv_ms"] > 0 and cp["device_ms"] > 0 and gv["device_ms"] > 0
        res.append((vt, cp, gv))
    eng.close()
    for a, b in zip(res[0], res[1]):
        for k in a:
            if not k.endswith("_ms"):
                assert np.array_equal(a[k], b[k]), k
    assert np.abs(res[0][0]["pv"]).max() > 0 and (res[0][2]["vdep"] > 0).any()
