"""GPU: the engine's own multi-rank protocol with two processes on ONE GPU.

RCCL refuses two ranks on the same device, so on a one-GPU box the reduction runs through the engine's second
transport, the host-supplied all-reduce of fpx_comm_init_host (what an MPI host passes; here gloo).  Everything else
is the code the 8-GPU run executes: particle shards with global particle numbers as RNG keys, per-rank partial sums in
device memory, receive buffers for the reduced grids, two output times with cumulative deposition grids; the output files
written from the receive buffers (reduced = 1) and the rule that says when those buffers are stale."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %(root)r)
    import numpy as np
    from flexpart_amd import sharding, synthetic as syn
    from flexpart_amd.engine import Engine, RNG_PHILOX

    def scenario():
        sc = syn.small(n=6000, nx=48, ny=32, nz=36, nsteps=4, ctl=5.0, ifine=4, cblflag=1)
        sc.update(lsettling=1, drydep=1, drydepspec=np.array([1], np.int32), density=np.array([2000.0]),
                  dquer=np.array([8.0]), vsetaver=np.array([-0.004]), cunningham=np.array([1.02]),
                  decay=np.array([1.0e-6]), xmass=np.array([1.0]))
        syn.add_outgrid(sc)
        syn.add_wet(sc, gas=False)
        syn.add_outgrid_nest(sc)
        syn.add_receptors(sc)
        return sc

    def run(eng, allreduce, sort_at=None):
        outs = []
        for out_time in range(2):               # two output times, two synchronisation steps each
            for k in range(2):
                if eng.itime != 0:
                    eng.wetdepo()
                eng.step()
                eng.conccalc(eng.itime, 1.0)
            if sort_at == out_time:
                eng.sort()
            g, d = eng.grids(allreduce=allreduce, clear=True)     # clear: gridunc only (concoutput.f90:719-720)
            w = eng.wetgrid(allreduce=allreduce)
            gn, dn, wn = eng.grids_nest(allreduce=allreduce, clear=True)
            r = eng.receptors(allreduce=allreduce, clear=True)
            outs.append(dict(gridunc=g, drygridunc=d, wetgridunc=w, griduncn=gn, drygriduncn=dn, wetgriduncn=wn, creceptor=r))
        return outs
""")

WORKER = COMMON + textwrap.dedent("""
    import torch.distributed as dist
    rank = int(sys.argv[1])
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=2)
    sc = scenario()
    mine = sharding.shard_scenario(sc, 2, rank)
    eng = Engine(mine, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_PHILOX, seed=4711, **%(ekw)r)   # particle_base from the shard
    eng.comm_init_host(dist, 2, rank)
    outs = run(eng, True, sort_at=0 if rank == 1 else None)
    state = eng.download()
    np.savez(%(out)r + f"_rank{rank}.npz", x=state["xtra1"], z=state["ztra1"], itra1=state["itra1"], m=state["xmass1"],
             blended=eng.info("blended_steps"), **{f"o{i}_{k}": v for i, o in enumerate(outs) for k, v in o.items()})
    eng.close()
    dist.barrier()
    dist.destroy_process_group()
""")

SERIAL = COMMON + textwrap.dedent("""
    sc = scenario()
    eng = Engine(sc, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_PHILOX, seed=4711, **%(ekw)r)
    outs = run(eng, False)
    state = eng.download()
    np.savez(%(out)r + "_serial.npz", x=state["xtra1"], z=state["ztra1"], itra1=state["itra1"], m=state["xmass1"],
             blended=eng.info("blended_steps"), **{f"o{i}_{k}": v for i, o in enumerate(outs) for k, v in o.items()})
    eng.close()
""")


@pytest.mark.parametrize("blend", ["off", "forced_on", "auto_from_the_global_count"])
def test_two_ranks_one_gpu_two_output_times(built, tmp_path, blend):
    """blend: the time-blended wind packs round differently from the plain gather, so whether a step uses them must not
    depend on the rank count: fpx_config.blend_mode (1 = on) or, in the automatic mode, the run's particle count over ALL
    ranks (global_particles: 4e7 here, above the threshold on every rank although each holds 3000 particles) -- the sharded
    and the single-rank run stay bitwise equal with the blend ON (README_PARALLEL.md:189-192), and it did run (blended_steps).
    mpi_mod.f90:2451-2492 through the engine: two ranks share one cloud (contiguous ranges of particle numbers,
    README_PARALLEL.md:60-67), reduce gridunc / drygridunc / wetgridunc (+ nested grids, creceptor) at two output
    times into receive buffers and keep accumulating their partial sums in between.  (i) With the counter RNG keyed on
    the global particle number every particle ends exactly where the single-rank run puts it.  (ii) The sums at BOTH
    output times equal the single-rank grids: an in-place reduction (round 1) fails the second one by the first total."""
    out = str(tmp_path / "mr")
    port = 33500 + (os.getpid() % 2000)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    ekw = {"off": {}, "forced_on": {"blend_mode": 1}, "auto_from_the_global_count": {"global_particles": 40000000}}[blend]
    ws = tmp_path / "worker.py"
    ws.write_text(WORKER % dict(root=ROOT, port=port, out=out, ekw=ekw))
    ss = tmp_path / "serial.py"
    ss.write_text(SERIAL % dict(root=ROOT, out=out, ekw=ekw))
    procs = [subprocess.Popen([sys.executable, str(ws), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    r = subprocess.run([sys.executable, str(ss)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    a, b, s = (np.load(out + f"_{t}.npz") for t in ("rank0", "rank1", "serial"))
    for d in (a, b, s):
        assert (int(d["blended"]) > 0) == (blend != "off"), blend
    # (i) sharding does not change any particle (counter RNG keyed on the global number; rank 1 even re-sorted its slots)
    for k in ("x", "z", "itra1"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), s[k]), k
    assert np.array_equal(np.concatenate([a["m"], b["m"]], axis=1), s["m"])
    # (ii) both output times; every rank received the same sums
    for i in range(2):
        for k in ("gridunc", "drygridunc", "wetgridunc", "griduncn", "drygriduncn", "wetgriduncn", "creceptor"):
            want, g0, g1 = s[f"o{i}_{k}"], a[f"o{i}_{k}"], b[f"o{i}_{k}"]
            assert want.sum() > 0, (i, k)
            assert np.array_equal(g0, g1), (i, k)
            tol = 1e-12 if k in ("gridunc", "griduncn", "creceptor") else 2e-5     # f32 atomics sum in another order
            assert np.abs(g0 - want).max() <= tol * want.max(), (i, k, np.abs(g0 - want).max() / want.max())
    for k in ("drygridunc", "wetgridunc", "drygriduncn", "wetgriduncn"):
        assert s[f"o1_{k}"].sum() > 1.2 * s[f"o0_{k}"].sum(), k        # the deposition grids did accumulate over the run
    assert s["o1_gridunc"].sum() < 1.5 * s["o0_gridunc"].sum()          # gridunc was zeroed after the first output


REDIST_WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %(root)r)
    import numpy as np
    import torch.distributed as dist
    from flexpart_amd import sharding, synthetic as syn
    from flexpart_amd.engine import Engine, RNG_PHILOX
    rank = int(sys.argv[1])
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=2)
    n = (260000, 120000)[rank]
    sc = syn.small(n=n, nx=48, ny=32, nz=36, nsteps=2, ctl=5.0, ifine=4, cblflag=1, seed=100 + rank)
    eng = Engine(sc, compute_real_bytes=8, host_real_bytes=8, rng_mode=RNG_PHILOX, seed=4711, max_particles=300000,
                 particle_base=rank * 300000)
    eng.upload_particles_from_scenario(sc)
    eng.step()                                   # a step first: some particles leave, the slots get sorted on rank 0
    if rank == 0:
        eng.sort()
    before = eng.download()
    itime = eng.itime
    role, peer, nt = sharding.redistribute_particles(dist, eng, itime)
    after = eng.download(0, 300000)
    stats = eng.step()                           # the received particles advance with everything else
    np.savez(%(out)r + f"_rank{rank}.npz", role=role, peer=peer, nt=nt, n_after=eng.n, itime=itime, due=stats["n_due"],
             bx=before["xtra1"], by=before["ytra1"], bz=before["ztra1"], bi=before["itra1"], bm=before["xmass1"],
             ax=after["xtra1"], ay=after["ytra1"], az=after["ztra1"], ai=after["itra1"], am=after["xmass1"])
    eng.close()
    dist.barrier()
    dist.destroy_process_group()
""")


def test_two_ranks_level_their_particle_counts(built, tmp_path):
    """mpif_calculate_part_redist + mpif_redist_part (mpi_mod.f90:566-856) between two processes on one GPU, the transport
    being the host's (gloo send / recv of the one packed message): 260000 and 120000 particles -> the plan moves 70000; the
    particles alive at itime are the same set before and after (position, height and mass of each), the counts are levelled,
    and the next step advances every one of them."""
    out = str(tmp_path / "rd")
    port = 35500 + (os.getpid() % 2000)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    ws = tmp_path / "redist_worker.py"
    ws.write_text(REDIST_WORKER % dict(root=ROOT, port=port, out=out))
    procs = [subprocess.Popen([sys.executable, str(ws), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    a, b = (np.load(out + f"_rank{r}.npz") for r in (0, 1))
    assert (int(a["role"]), int(a["peer"]), int(a["nt"])) == (1, 1, 70000)
    assert (int(b["role"]), int(b["peer"]), int(b["nt"])) == (2, 0, 70000)
    itime = int(a["itime"])

    def alive(d, p):
        m = d[p + "i"] == itime
        rows = np.stack([d[p + "x"][m], d[p + "y"][m], d[p + "z"][m], d[p + "m"].reshape(-1, d[p + "i"].size)[0][m]], axis=1)
        return rows[np.lexsort(rows.T[::-1])]
    before = np.concatenate([alive(a, "b"), alive(b, "b")])
    after = np.concatenate([alive(a, "a"), alive(b, "a")])
    before, after = (v[np.lexsort(v.T[::-1])] for v in (before, after))
    assert before.shape == after.shape and np.array_equal(before, after)
    na, nb = int((a["ai"] == itime).sum()), int((b["ai"] == itime).sum())
    nb0 = int((b["bi"] == itime).sum())
    assert nb > nb0 and nb - nb0 <= 70000 and int(a["n_after"]) == 260000 - 70000
    assert int(a["due"]) == na and int(b["due"]) == nb                         # every particle, received ones included, advanced


def test_bench_two_ranks_is_the_single_rank_job(built, tmp_path):
    """bench.py --gpus 2 as the driver will start it (here: bench.py launches its two ranks itself, as fresh child processes;
    on this one-GPU box they share the device and reduce over the host transport -- on a node each has its own GPU and RCCL):
    the line reports two ranks, every particle of the one cloud is alive on some rank, and the all-reduced concentration
    grid is the single-rank run's (mpi_mod.f90:2451-2492, timemanager_mpi.f90:552-562)."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    lines = {}
    for n in (1, 2):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--config", "4", "--particles", "2e6", "--steps", "2", "--warmup", "1",
               "--no-cpu-baseline", "--no-pmc"]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines[n] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    one, two = lines[1], lines[2]
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["config"]["live_particles_all_ranks"] == one["config"]["live_particles_all_ranks"] == 2000000
    assert two["config"]["particles_per_gpu"] == 1000000 and two["config"]["reduction_transport"] is not None
    assert two["config"]["time_blended_packs"] == one["config"]["time_blended_packs"]
    a, b = one["config"]["gridunc_sum_all_ranks"], two["config"]["gridunc_sum_all_ranks"]
    assert a > 0 and abs(a - b) <= 1e-6 * a, (a, b)
    assert abs(two["config"]["particle_steps_timed"] - one["config"]["particle_steps_timed"]) <= 2


# ---- the reduced = 1 writers and the rule that says when a reduction is stale ---------------------------------------
# One script per leg, started as rank 0 and rank 1 of a two-rank run and once more as a run of its own (world = 1).  Each
# process pickles what it wrote and what it was refused; the test compares.

REDUCED_COMMON = textwrap.dedent("""
    import pickle
    sys.path.insert(1, %(tests)r)
    from flexpart_amd._lib import FpxError
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
    files, refused, counter = {}, {}, [0]

    def fresh():                                  # every call of a writer gets a prefix of its own
        counter[0] += 1
        d = %(out)r + f"_w{world}r{rank}_{counter[0]:03d}"
        os.mkdir(d)
        return d + os.sep

    def refuses(what, call):
        # FPX_ERR_STATE with the text that names the getter to call first -- and nothing else counts
        try:
            call()
            refused[what] = "the call succeeded"
        except FpxError as e:
            refused[what] = True if e.code == -3 and "reduced = 1 needs" in str(e) else str(e)

    def finish(**arrays):
        with open(%(out)r + f"_w{world}r{rank}.pkl", "wb") as f:
            pickle.dump(dict(files=files, refused=refused, **arrays), f)
        eng.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
""")

REDUCED_FORWARD = COMMON + REDUCED_COMMON + textwrap.dedent("""
    import calcfluxes_ref as cr
    from oracle import oracle as orc
    sc = scenario()
    sc.update(iflux=1, device_flux=1)
    if world > 1:
        sc = sharding.shard_scenario(sc, world, rank)
    eng = Engine(sc, compute_real_bytes=8, host_real_bytes=4, rng_mode=RNG_PHILOX, seed=4711)   # concoutput: 4-byte hosts only
    if world > 1:
        eng.comm_init_host(dist, world, rank)
    na, nc, mp, nsp, nzg, nyg, nxg = eng.gshape
    nyn, nxn = eng.gshape_nest[5:7]
    assert (na, nc, mp) == (1, 1, 1)
    OUTNUM = 2.0
    case = {False: syn.concoutput_case(nxg=nxg, nyg=nyg, nzg=nzg, nspec=nsp), True: syn.concoutput_case(nxg=nxn, nyg=nyn, nzg=nzg, nspec=nsp)}
    areas = (1.0e8 * (1.0 + (np.arange(nyg * nxg).reshape(nyg, nxg) %% 7) / 8.0),
             1.0e6 * (1.0 + (np.arange(nzg * nyg * nxg).reshape(nzg, nyg, nxg) %% 5) / 8.0),
             1.0e6 * (1.0 + (np.arange(nzg * nyg * nxg).reshape(nzg, nyg, nxg) %% 3) / 4.0))

    def conc(nest, reduced, wet=True, dry=True):
        prefix = fresh()
        eng.concoutput(3600, prefix, case[nest]["area"], case[nest]["volume"], outnum=OUTNUM, wetdep=wet, drydep=dry, nest=nest, reduced=reduced)
        return [open(prefix + "%%03d" %% (k + 1), "rb").read() for k in range(nsp)]

    def conc_oracle(nest, g, d, w):              # as tests/test_concoutput.py feeds the oracle
        c = case[nest]
        geom = c["outgeom"].copy(); geom[4] = OUTNUM
        co = dict(outgrid=np.array([nxn if nest else nxg, nyn if nest else nyg, nzg, nsp, 1, 1, 3600], np.int32), outgeom=geom,
                  outheight=c["outheight"], area=c["area"], volume=c["volume"], gridunc=g[0, 0, 0], wetgridunc=w[0, 0, 0], drygridunc=d[0, 0, 0])
        got = orc.co_oracle(co)
        return [got["_%%03d" %% (k + 1)] for k in range(nsp)]

    def flux(reduced):
        return open(eng.fluxoutput(eng.itime, fresh(), *areas, outstep=3600.0, bdate=syn.GV_BDATE, reduced=reduced), "rb").read()

    def flux_ref(fl):                            # as tests/test_calcfluxes.py feeds the restatement's writer
        return cr.fluxoutput(fl, "r4", eng.itime, *areas, 3600.0)

    def sync_step():
        if eng.itime != 0:
            eng.wetdepo()
        eng.step()
        eng.conccalc(eng.itime, 1.0)

    def reduce_all():
        g, d = eng.grids(allreduce=True)
        w = eng.wetgrid(allreduce=True)
        gn, dn, wn = eng.grids_nest(allreduce=True)
        return dict(g=g, d=d, w=w, gn=gn, dn=dn, wn=wn, fl=eng.get_flux(allreduce=True))

    ck = %(out)r + f"_w{world}r{rank}.ckpt"
    if world == 1:
        # a single rank: reduced = 1 needs no call before it and writes the partial sums, which are the sums
        for _ in range(2):
            sync_step()
        eng.checkpoint_write(ck)
        for nest in (False, True):
            files[f"conc{nest:d}_red"] = conc(nest, True)
            files[f"conc{nest:d}_own"] = conc(nest, False)
        files["flux_own"] = flux(False)          # zeroes flux ...
        eng.checkpoint_read(ck)                  # ... and this brings it back
        files["flux_red"] = flux(True)
        finish()
        sys.exit(0)

    for nest in (False, True):
        refuses(f"before the first all-reduce: concoutput nest={nest:d}", lambda: conc(nest, True))
    refuses("before the first all-reduce: fluxoutput", lambda: flux(True))
    for _ in range(2):
        sync_step()
    eng.checkpoint_write(ck)
    red = reduce_all()
    for nest in (False, True):
        files[f"conc{nest:d}_own"] = conc(nest, False)
        files[f"conc{nest:d}_red"] = conc(nest, True)
        files[f"conc{nest:d}_ref"] = conc_oracle(nest, *((red["gn"], red["dn"], red["wn"]) if nest else (red["g"], red["d"], red["w"])))
    files["flux_ref"] = flux_ref(red["fl"])
    files["flux_red"] = flux(True)
    refuses("fluxoutput has zeroed flux: fluxoutput", lambda: flux(True))

    # conccalc moves gridunc / griduncn on; the sums of the deposition grids stay good
    eng.conccalc(eng.itime, 1.0)
    for nest in (False, True):
        refuses(f"conccalc: concoutput nest={nest:d}", lambda: conc(nest, True, wet=False, dry=False))
    reduce_all()
    for nest in (False, True):
        conc(nest, True)                         # everything is valid again
    # a step moves drygridunc / drygriduncn and flux on, and nothing else
    eng.step()
    for nest in (False, True):
        refuses(f"step: concoutput drydep nest={nest:d}", lambda: conc(nest, True, wet=False, dry=True))
        conc(nest, True, wet=True, dry=False)
    refuses("step: fluxoutput", lambda: flux(True))
    # wetdepo moves wetgridunc / wetgriduncn on, and nothing else
    eng.wetdepo()
    for nest in (False, True):
        refuses(f"wetdepo: concoutput wetdep nest={nest:d}", lambda: conc(nest, True, wet=True, dry=False))
        conc(nest, True, wet=False, dry=False)
    # a restored checkpoint replaces every partial sum
    reduce_all()
    for nest in (False, True):
        conc(nest, True)
    eng.checkpoint_read(ck)
    for nest in (False, True):
        refuses(f"checkpoint_read: concoutput nest={nest:d}", lambda: conc(nest, True, wet=False, dry=False))
        refuses(f"checkpoint_read: concoutput drydep nest={nest:d}", lambda: conc(nest, True, wet=False, dry=True))
        refuses(f"checkpoint_read: concoutput wetdep nest={nest:d}", lambda: conc(nest, True, wet=True, dry=False))
    refuses("checkpoint_read: fluxoutput", lambda: flux(True))
    # flux is what it was when the reduced file was written: the partial sums of this rank, through the same writer
    own = eng.get_flux()
    files["flux_own_ref"] = flux_ref(own)
    files["flux_own"] = flux(False)
    finish(own=own, **red)
""")

REDUCED_BACKWARD = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %(root)r)
    import numpy as np
    from flexpart_amd import sharding
""") + REDUCED_COMMON + textwrap.dedent("""
    import initcond_ref as ir
    import test_initcond as tic
    sc = tic.ic_scenario(1)
    if world > 1:
        sc = sharding.shard_scenario(sc, world, rank)
    eng = tic.make_engine(sc, 8, 8)
    if world > 1:
        eng.comm_init_host(dist, world, rank)
    rho_rel = np.array([1.125, 0.9375, 1.0625])

    def write(reduced):
        return [open(n, "rb").read() for n in eng.initial_cond_output(eng.itime, fresh(), ind_rel=1, rho_rel=rho_rel, reduced=reduced)]

    if world == 1:
        for _ in range(tic.NSTEPS):
            eng.step()
        eng.initcond_finish()
        files["red"] = write(True)
        files["own"] = write(False)
        finish()
        sys.exit(0)

    ck = %(out)r + f"_w{world}r{rank}.ckpt"
    refuses("before the first all-reduce", lambda: write(True))
    for _ in range(tic.NSTEPS):
        eng.step()
    eng.initcond_finish()
    eng.checkpoint_write(ck)
    red = eng.get_initcond(allreduce=True)
    own = eng.get_initcond()
    files["own"] = write(False)
    files["red"] = write(True)
    files["ref"] = ir.initial_cond_output(red, "r8", eng.itime, sc["xmass"], 1, rho_rel)
    eng.step()
    refuses("step", lambda: write(True))
    eng.get_initcond(allreduce=True)
    write(True)
    eng.initcond_finish()
    refuses("initcond_finish", lambda: write(True))
    eng.get_initcond(allreduce=True)
    write(True)
    eng.checkpoint_read(ck)
    refuses("checkpoint_read", lambda: write(True))
    assert np.array_equal(eng.get_initcond(), own)
    finish(own=own, red=red)
""")


def run_reduced(tmp_path, script, port):
    """rank 0 and rank 1 of a two-rank run and a single-rank run of `script`, side by side: what each pickled."""
    import pickle
    out = str(tmp_path / "rw")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    ws = tmp_path / "reduced_worker.py"
    ws.write_text(script % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), port=port, out=out))
    procs = [subprocess.Popen([sys.executable, str(ws), str(r), str(w)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r, w in ((0, 2), (1, 2), (0, 1))]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return [pickle.load(open(out + f"_w{w}r{r}.pkl", "rb")) for r, w in ((0, 2), (1, 2), (0, 1))]


def test_reduced_forward_files_and_staleness(built, tmp_path):
    """fpx_concoutput (mother and nested output grid, with both deposition grids) and fpx_fluxoutput with reduced = 1 on two
    ranks (concoutput_mpi.f90:279,298: the root writes from gridunc0 / drygridunc0 / wetgridunc0): both ranks write the same
    bytes; they are the bytes the reference writers make of the reduced arrays the rank fetched (no tolerance: the same
    numbers go into both); reduced = 0 on the same rank writes other bytes; the grids hold data.  Then the rule that says
    when a receive buffer is stale, as the engine has it: every case below is refused with FPX_ERR_STATE, and the calls the
    same event must not touch still succeed (the worker would fail).  A single rank needs no reduction and writes the same
    bytes either way."""
    a, b, s = run_reduced(tmp_path, REDUCED_FORWARD, 39500 + (os.getpid() % 2000))
    for r in (a, b):
        f = r["files"]
        for key in ("conc0", "conc1", "flux"):
            assert f[key + "_red"] == f[key + "_ref"], key
            assert f[key + "_red"] != f[key + "_own"], key
        assert f["flux_own"] == f["flux_own_ref"]
    for key in ("conc0_red", "conc1_red", "flux_red"):
        assert a["files"][key] == b["files"][key], key
    assert (a["g"] > 0).sum() > 100 and (a["gn"] > 0).sum() > 100
    for k in ("d", "w", "dn", "wn", "fl"):
        assert np.count_nonzero(a[k]) > 0, k
    for k in ("g", "d", "w", "gn", "dn", "wn", "fl"):
        assert np.array_equal(a[k], b[k]), k
    assert np.count_nonzero(a["own"]) > 0 and np.count_nonzero(b["own"]) > 0 and np.array_equal(a["own"] + b["own"], a["fl"])
    want = {f"{why}: concoutput nest={n}" for why in ("before the first all-reduce", "conccalc") for n in (0, 1)}
    want |= {f"{why}: fluxoutput" for why in ("before the first all-reduce", "fluxoutput has zeroed flux", "step", "checkpoint_read")}
    want |= {f"step: concoutput drydep nest={n}" for n in (0, 1)} | {f"wetdepo: concoutput wetdep nest={n}" for n in (0, 1)}
    want |= {f"checkpoint_read: concoutput{dep} nest={n}" for dep in ("", " drydep", " wetdep") for n in (0, 1)}
    for r in (a, b):
        assert set(r["refused"]) == want
        assert all(v is True for v in r["refused"].values()), r["refused"]
    f = s["files"]
    for key in ("conc0", "conc1", "flux"):
        assert f[key + "_red"] == f[key + "_own"] and all(len(x) > 200 for x in ([f[key + "_red"]] if key == "flux" else f[key + "_red"])), key


def test_reduced_backward_files_and_staleness(built, tmp_path):
    """fpx_initial_cond_output with reduced = 1 on two ranks of the backward run of tests/test_initcond.py, after
    fpx_get_initcond(allreduce = 1): the same three properties against the restatement's writer, and the staleness rule of
    init_cond: a step, fpx_initcond_finish and a restored checkpoint each make the reduction stale."""
    a, b, s = run_reduced(tmp_path, REDUCED_BACKWARD, 41500 + (os.getpid() % 2000))
    for r in (a, b):
        f = r["files"]
        assert f["red"] == f["ref"] and f["red"] != f["own"] and len(f["red"]) == 2
        assert set(r["refused"]) == {"before the first all-reduce", "step", "initcond_finish", "checkpoint_read"}
        assert all(v is True for v in r["refused"].values()), r["refused"]
    assert a["files"]["red"] == b["files"]["red"]
    assert np.array_equal(a["red"], b["red"]) and np.count_nonzero(a["red"]) > 50
    assert np.count_nonzero(a["own"]) > 0 and np.count_nonzero(b["own"]) > 0
    assert s["files"]["red"] == s["files"]["own"] and all(len(x) > 200 for x in s["files"]["red"])
