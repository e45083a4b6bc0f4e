"""The output-grid scatter kernels, cell by cell.

Every number a user gets (gridunc, drygridunc, wetgridunc, their nested twins, creceptor) passes through the wave-level
code of flexpart_amd/csrc/fpx_device.hpp: wave_kernel_add / wave_total (lanes grouped by target cell, nine DPP reductions
into the 3 x 3 neighbourhood) and wave_run_add (segmented shuffle reduction).  The whole-run tests of test_gpu_parity.py
see it in max norm relative to the largest cell; here a cloud is laid out wave by wave (tests/scatter_ref.py), the
kernels are called alone (Engine.conccalc, Engine.wetdepo) and every cell is compared:

  * conccalc with dyadic positions and masses: every partial sum is exactly representable, so the device must equal the
    exact sums BIT FOR BIT in both real kinds (np.array_equal, no tolerance);
  * receptors, wet and dry deposition: derived per-cell bounds (DESIGN.md "Scatter kernels cell by cell" has the
    derivations and the worst observed error / bound ratios).

The CPU tests pin the numpy restatement to the C oracle bit for bit and check the exactness precondition.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import scatter_ref as sr

KINDS = {"r8": np.float64, "r4": np.float32}
# (one hour of scavenging: the oracle's median deposit is then 63 % of the mass for the aerosol and 22 % for the gas, and nine
# particles in ten lose a tenth or more; with 900 s the gas loses 7 %, too little for the precondition of the wet test)
LTSAMPLE, LOUTNEXT = 3600, 10800


@functools.lru_cache(maxsize=None)
def _cloud(wet=False):
    return sr.pattern_cloud(wet=wet)


@functools.lru_cache(maxsize=None)
def _exact(kind, luse, n=None):
    """Exact gridunc, griduncn (flat, float64) of the first n particles of the pattern cloud: computed once, never modified."""
    cloud = _cloud()
    sc = sr.scenario(cloud, lusekerneloutput=luse)
    p = cloud.arrays(n)
    out = tuple(sr.exact_gridunc(sc, p, KINDS[kind], nest=nest) for nest in (False, True))
    for a in out:
        a.setflags(write=False)
    return out


def _oracle(sc, cloud, kind):
    from oracle.oracle import Oracle
    osc = dict(sc)
    osc.update(cloud.oracle_view())
    return Oracle(osc, kind)


def _orc_wetdepo(orc, ltsample):
    """orc_wetdepo as Oracle.step calls it -> (xmass1 before, after) as float64."""
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    before = orc.xmass1.astype(np.float64)
    orc.lib.orc_wetdepo(orc.h, sr.ITIME, int(ltsample), LOUTNEXT, orc.n, vp(orc.x), vp(orc.y), vp(orc.z), vp(orc.itra1),
                        vp(orc.itramem), vp(orc.npoint), vp(orc.nclass), vp(orc.xmass1))
    return before, orc.xmass1.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against the C oracle, and the exactness precondition
# ------------------------------------------------------------------------------------------------------------------
def test_pattern_cloud_layout():
    cloud = _cloud()
    assert cloud.n % 64 == 1 and cloud.n <= 30 * 64
    starts = sorted(a for a, _ in cloud.ranges.values())
    assert starts == list(range(0, cloud.n, 64))          # one wave per pattern, the tail alone in the last
    k = cloud.ranges["inactive_even_lanes"][0]
    assert cloud.kinds[k] != "ok" and cloud.kinds[k + 63] == "ok"          # lane 0 of that wave is inactive ...
    k = cloud.ranges["inactive_odd_lanes"][0]
    assert cloud.kinds[k] == "ok" and cloud.kinds[k + 63] != "ok"          # ... and lane 63 of this one
    for kind in sr.INACTIVE:                                               # every kind on an even and on an odd lane
        assert {i % 2 for i, v in enumerate(cloud.kinds) if v == kind} == {0, 1}, kind


@pytest.mark.parametrize("luse", [1, 0], ids=["kernel", "nokernel"])
def test_exactness_precondition(luse):
    """Every contribution is an integer multiple of the quantum, every cell's sum of magnitudes stays below 2**24 quanta
    (so every partial sum in any order is a float32), and the f32 and fp64 evaluations of the restatement agree exactly."""
    cloud = _cloud()
    sc = sr.scenario(cloud, lusekerneloutput=luse)
    p = cloud.arrays()
    for nest in (False, True):
        i8, v8 = sr.conccalc_contribs(sc, p, np.float64, nest=nest)
        i4, v4 = sr.conccalc_contribs(sc, p, np.float32, nest=nest)
        assert np.array_equal(i8, i4) and np.array_equal(v8, v4.astype(np.float64))
        q = v8 / sr.QUANTUM
        assert np.array_equal(q, np.round(q)) and q.min() >= 0
        size = sr.grid_size(sc, nest)
        assert sr.sum_cells(i8, np.abs(q), size).max() < 2.0 ** 24
        assert len(i8) > (1000 if not nest else 300) and i8.min() >= 0 and i8.max() < size
    assert np.array_equal(_exact("r8", luse)[0], _exact("r4", luse)[0]) and np.array_equal(_exact("r8", luse)[1], _exact("r4", luse)[1])


@pytest.mark.parametrize("luse", [1, 0], ids=["kernel", "nokernel"])
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_restatement_matches_oracle_conccalc(kind, luse):
    """Oracle.sample(0.5) on the pattern cloud: gridunc, griduncn and creceptor bit for bit."""
    cloud = _cloud()
    sc = sr.scenario(cloud, lusekerneloutput=luse)
    orc = _oracle(sc, cloud, kind)
    orc.sample(sr.WEIGHT)
    og, _ = orc.grids()
    ogn, _, _ = orc.grids_nest()
    want, wantn = _exact(kind, luse)
    assert og.sum() > 0 and ogn.sum() > 0
    assert np.array_equal(og.ravel(), want) and np.array_equal(ogn.ravel(), wantn)
    # (the receptor kernel has no class guard: the oracle's view of the cloud, where the guarded lanes are not due)
    rec = sr.receptor_serial(sc, cloud.oracle_view(), KINDS[kind])
    assert rec.max() > 0 and np.array_equal(orc.receptors(), rec)


@pytest.mark.parametrize("luse", [1, 0], ids=["kernel", "nokernel"])
@pytest.mark.parametrize("wet", ["aerosol", "gas"])
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_restatement_matches_oracle_wetdepo(kind, wet, luse):
    """orc_wetdepo on the pattern cloud with a saturating sampling time (the deposit is then xmass * grfraction, free of
    transcendental functions): particle masses, wetgridunc and wetgriduncn bit for bit, the grids accumulated serially as the
    reference does."""
    R = KINDS[kind]
    cloud = _cloud(True)
    sc = sr.scenario(cloud, wet=wet, lusekerneloutput=luse)
    orc = _oracle(sc, cloud, kind)
    _, after = _orc_wetdepo(orc, sr.SATURATING_LTSAMPLE)
    p = cloud.oracle_view()
    dep, want_after = sr.wet_deposit_saturated(sc, p, R)
    assert np.array_equal(after, want_after.astype(np.float64))
    assert (dep > 0).sum() > 1000
    _, nage, kp, nc, _, _ = sr._planes(sc, p, sr.ITIME)
    species = [ks for ks in range(sr.NSPEC) if sc["wetdepspec"][ks]]
    for nest, got in ((False, orc.wetgrid()), (True, orc.grids_nest()[2])):
        want = sr.serial_depo_grid(sc, p["xtra1"], p["ytra1"], R, dep, species, nage, kp, nc, nest=nest)
        assert got.sum() > 0 and np.array_equal(got.ravel(), want)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _engine(sc, kind):
    from flexpart_amd.engine import Engine
    rb = 8 if kind == "r8" else 4
    return Engine(sc, compute_real_bytes=rb, host_real_bytes=rb)


@pytest.mark.gpu
@pytest.mark.parametrize("luse", [1, 0], ids=["kernel", "nokernel"])
@pytest.mark.parametrize("order", ["unsorted", "sorted"])
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_conccalc_exact(built, kind, order, luse):
    """k_conccalc alone on the pattern cloud: gridunc and griduncn equal the exact sums in every cell of the full 7-D arrays,
    bit for bit (r4: wave_kernel_add<float> / wave_total<float>; r8: the two-half fp64 DPP moves and readlane).  A second
    call doubles every cell exactly.  Then the first 256 + 3 and 64 * 5 + 63 particles only: a block boundary and partial
    last waves."""
    cloud = _cloud()
    sc = sr.scenario(cloud, lusekerneloutput=luse)
    want, wantn = _exact(kind, luse)
    eng = _engine(sc, kind)
    try:
        if order == "sorted":
            eng.sort()
        eng.conccalc(sr.ITIME, sr.WEIGHT)
        g, d = eng.grids()
        gn, dn, wn = eng.grids_nest()
        assert want.max() > 0 and wantn.max() > 0
        assert np.array_equal(g.ravel(), want), _diff(g.ravel(), want)
        assert np.array_equal(gn.ravel(), wantn), _diff(gn.ravel(), wantn)
        assert not d.any() and not dn.any() and not wn.any()
        eng.conccalc(sr.ITIME, sr.WEIGHT)
        assert np.array_equal(eng.grids()[0].ravel(), 2.0 * want) and np.array_equal(eng.grids_nest()[0].ravel(), 2.0 * wantn)
        for n in (256 + 3, 64 * 5 + 63):
            eng.grids(clear=True); eng.grids_nest(clear=True)
            eng.set_numpart(n)
            eng.conccalc(sr.ITIME, sr.WEIGHT)
            w, wn_ = _exact(kind, luse, n)
            assert np.array_equal(eng.grids()[0].ravel(), w) and np.array_equal(eng.grids_nest()[0].ravel(), wn_), n
    finally:
        eng.close()


def _diff(got, want):
    bad = np.flatnonzero(got != want)
    return f"{len(bad)} cells differ; first: {[(int(i), float(got[i]), float(want[i])) for i in bad[:8]]}"


def _ratio(err, bound):
    """Worst error / bound over the cells with a bound; a cell without one must be met exactly."""
    assert not err[bound == 0].any(), "a cell that receives nothing is not zero"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_receptors_per_receptor(built, kind):
    """The receptor kernel (wave_run_add) per (species, receptor) on hit / miss lane patterns: all 64, alternating, exactly two,
    exactly three, lanes 0 and 63 only, a run broken by one miss.  Every accept test keeps a margin of 1e-3, so device and
    restatement take the same decisions.  |dev - fsum| <= (n_hit + 16) eps sum|c_p|: the summation in any order, plus the
    roughly ten roundings of one contribution (the device contracts and orders them differently)."""
    R = KINDS[kind]
    cloud = sr.receptor_cloud()
    sc = sr.scenario(cloud)
    p = cloud.arrays()
    t = sr.receptor_terms(sc, p, R)
    assert t["margin"].min() >= 1e-3, t["margin"].min()
    nrec = t["hit"].shape[0]
    for r in range(nrec):
        assert np.array_equal(t["hit"][r], cloud.want_hit & (cloud.receptor_of == r))
    eng = _engine(sc, kind)
    try:
        eng.conccalc(sr.ITIME, sr.WEIGHT)
        got = eng.receptors()
    finally:
        eng.close()
    worst = 0.0
    for ks in range(sr.NSPEC):
        for r in range(nrec):
            c = t["c"][ks, r][t["hit"][r]].astype(np.float64)
            bound = (len(c) + 16) * sr.eps_of(R) * math.fsum(np.abs(c))
            err = abs(got[ks, r] - math.fsum(c))
            worst = max(worst, err / bound)
            print(f"receptor {r} species {ks}: n_hit {len(c)} err/bound {err / bound:.3f}")
            assert len(c) >= 2 and err <= bound, (ks, r, err, bound)
    print(f"test_receptors_per_receptor[{kind}] worst err/bound {worst:.3f}")


def _depo_check(sc, x, y, R, D, species, m_before, nage, kp, nc, dev, *, nest, kind, mass_eps):
    """Per-cell bound of a deposition grid: 2**-24 (n_c + 2) A_c for the float32 sums in any order and the rounding
    of a contribution, plus 3 mass_eps sum |w| m for the rounding of the mass difference the deposit is taken from."""
    t = sr.depo_contribs(sc, x, y, R, D, species, nage, kp, nc, nest=nest, kind=kind)
    size = sr.grid_size(sc, nest, levels=False)
    want = sr.sum_cells(t["idx"], t["val"], size)
    A = sr.sum_cells(t["idx"], np.abs(t["val"].astype(np.float64)), size)
    n_c = sr.count_cells(t["idx"], size)
    M = sr.sum_cells(t["idx"], np.abs(t["w"]) * np.abs(m_before[t["species"], t["particle"]]), size)
    bound = 2.0 ** -24 * (n_c + 2) * A + 3.0 * mass_eps * M
    err = np.abs(dev.ravel() - want)
    ratio = _ratio(err, bound)
    planes = size // (sr._geom(sc, R, nest)["numx"] * sr._geom(sc, R, nest)["numy"])
    perr = np.abs(dev.reshape(planes, -1).sum(axis=1) - want.reshape(planes, -1).sum(axis=1))
    pratio = _ratio(perr, bound.reshape(planes, -1).sum(axis=1))
    return ratio, pratio, int((n_c > 0).sum()), int(n_c.max())


@pytest.mark.gpu
@pytest.mark.parametrize("wet", ["aerosol", "gas"])
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_wetdepo_scatter_per_cell(built, kind, wet):
    """k_wetdepo alone on the pattern cloud over raining columns: every cell of wetgridunc and wetgriduncn against the exact sum
    of float32(D_p w) with the restatement's weights.  D_p = mass before - mass after: in r8 from the oracle (the device's masses
    are pinned to it at 1e-11), in r4 from the device's own masses (the f32 scavenging coefficient differs from the oracle's by
    up to 2e-3).  Bound per cell: 2**-24 ((n_c + 2) A_c + 3 sum |w| m [r4 only]); a cell that receives nothing is exactly 0."""
    R = KINDS[kind]
    cloud = _cloud(True)
    sc = sr.scenario(cloud, wet=wet)
    p = cloud.arrays()
    m0 = p["xmass1"].astype(R).astype(np.float64)
    orc = _oracle(sc, cloud, kind)
    before_o, after_o = _orc_wetdepo(orc, LTSAMPLE)
    D_o = before_o - after_o
    scav = D_o > 0
    assert scav.sum() > 1000 and (D_o[scav] >= 0.1 * before_o[scav]).sum() >= 0.5 * scav.sum(), \
        (scav.sum(), (D_o[scav] >= 0.1 * before_o[scav]).sum())
    eng = _engine(sc, kind)
    try:
        eng.wetdepo(sr.ITIME, LTSAMPLE, LOUTNEXT)
        got = eng.download()
        w = eng.wetgrid()
        wn = eng.grids_nest()[2]
    finally:
        eng.close()
    same = ~cloud.guarded                 # (a lane the oracle was not given as due -- the engine's guards -- is not compared)
    if kind == "r8":
        assert np.abs(got["xmass1"][:, same] - after_o[:, same]).max() <= 1e-11
        D = np.where(same[None, :], D_o, m0 - got["xmass1"])
    else:
        D = m0 - got["xmass1"]
        assert (np.abs(got["xmass1"][:, same] - after_o[:, same]) > 2e-3 * m0[:, same]).sum() <= 0.02 * cloud.n
    assert D.min() >= 0
    _, nage, kp, nc, _, _ = sr._planes(sc, p, sr.ITIME)
    species = [ks for ks in range(sr.NSPEC) if sc["wetdepspec"][ks]]
    live = (p["itra1"] != sr.DEAD) & (p["itra1"] <= sr.ITIME) & sr._in_domain(sc, p)
    assert not D[:, ~live].any()
    for nest, dev in ((False, w), (True, wn)):
        ratio, pratio, cells, nmax = _depo_check(sc, p["xtra1"], p["ytra1"], R, D, species, m0, nage, kp, nc, dev, nest=nest,
                                                 kind="wet", mass_eps=2.0 ** -24 if kind == "r4" else 0.0)
        print(f"test_wetdepo_scatter_per_cell[{kind}-{wet}] nest={nest}: {cells} cells, up to {nmax} contributions, "
              f"worst err/bound cell {ratio:.3f} plane {pratio:.3f}")
        assert cells > (150 if not nest else 60) and ratio <= 1.0 and pratio <= 1.0, (ratio, pratio)


def dry_scenario():
    """2000 particles drawn together over about 3 x 3 mother output cells (6 x 6 nested ones) below 2 href = 30 m; two of
    three species deposit; deposition velocities ten times the synthetic default (2 to 7 cm/s)."""
    n = 2000
    sc = sr.scenario(nspec=3)
    sc.update(drydep=1, drydepspec=np.array([1, 0, 1], np.int32), vdep=np.asarray(sc["vdep"]) * 10.0)
    u = [sr.syn._uniform01(n, 0xD0 + k) for k in range(4)]
    i = np.arange(n)
    sc.update(npart=n, xtra1=12.2 + 1.4 * u[0], ytra1=10.3 + 1.4 * u[1], ztra1=2.0 + 26.0 * u[2],
              itra1=np.full(n, sr.ITIME, np.int32), itramem=(sr.ITIME - np.where((i // 9) % 2, sr.OLD, sr.YOUNG)).astype(np.int32),
              npoint=(1 + i % 3).astype(np.int32), nclass=(1 + (i // 3) % 3).astype(np.int32),
              xmass1=(1.0 + np.arange(3)[:, None]) * (0.5 + u[3])[None, :])
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_drydepo_scatter_per_cell(built, kind):
    """One step with dry deposition (k_pbl_finish -> drydepo_particle<R, true>): every cell of drygridunc and drygriduncn
    against the exact sum of float32(D_p w), D_p = mass before - mass after and the position after the step both from the
    device (other tests pin them to the oracle).  Bound per cell: 2**-24 (n_c + 2) A_c + 3 eps_R sum |w| m; the plane sums
    within the summed bounds.  A particle that left the domain contributes nothing."""
    R = KINDS[kind]
    sc = dry_scenario()
    m0 = np.asarray(sc["xmass1"]).astype(R).astype(np.float64)
    eng = _engine(sc, kind)
    try:
        eng.step(sr.ITIME)
        got = eng.download()
        d = eng.grids()[1]
        dn = eng.grids_nest()[1]
    finally:
        eng.close()
    stays = got["itra1"] == sr.ITIME + int(sc["lsynctime"])
    assert stays.sum() >= 0.99 * len(stays)
    D = np.where(stays[None, :], m0 - got["xmass1"], 0.0)
    species = [0, 2]
    assert not D[1].any() and D.min() >= 0
    loss = (D[species] / m0[species])[:, stays]
    print(f"test_drydepo_scatter_per_cell[{kind}]: median loss {np.median(loss):.3f}")
    assert np.median(loss) >= 0.05
    p = {k: np.asarray(sc[k]) for k in ("itramem", "npoint", "nclass")}
    _, nage, kp, nc, _, _ = sr._planes(sc, p, sr.ITIME)
    for nest, dev in ((False, d), (True, dn)):
        ratio, pratio, cells, nmax = _depo_check(sc, got["xtra1"], got["ytra1"], R, D, species, m0, nage, kp, nc, dev, nest=nest,
                                                 kind="dry", mass_eps=sr.eps_of(R))
        print(f"test_drydepo_scatter_per_cell[{kind}] nest={nest}: {cells} cells, up to {nmax} contributions, "
              f"worst err/bound cell {ratio:.3f} plane {pratio:.3f}")
        assert cells > 100 and nmax > 10 and ratio <= 1.0 and pratio <= 1.0, (ratio, pratio)
