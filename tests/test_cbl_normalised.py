"""cbl() in normalised variables (fpx_device.hpp, FPX_CBL_NORMALISED; DESIGN.md "Round 10") through fpx_cbl_probe, which calls
cbl() the way the fp64 gas kernels of the Langevin loop do and carries both bodies: form 0 the one in the reference's
dimensional variables, form 1 the normalised one.

  1. Both forms against the truth on about 2e4 seeded points of what the loop hands over (draw).  The truth is a 50-digit
     (mpmath) evaluation of cbl.f90:70-210 at exactly these points, recorded in tests/golden/cbl_truth_50digits.npz: ath as a
     double and the rest to it, (|Phi| + |(C0/2) alfa Q|)/ptot, flagrein, and d = deltawa/sigmawa, deltawb/sigmawb.  The file
     holds results only; it carries the SHA-256 of the input array, which the test checks, so a draw that changed cannot be
     compared with it.  bth = sigmaw*sqrt(2/tlw) is evaluated here, at 50 digits.
     The error of ath is taken relative to (|Phi| + |(C0/2) alfa Q|)/ptot of the truth and that of bth relative to bth.  The
     normalised form's worst error may be at most twice the dimensional form's on the same points: the two forms round a
     different handful of products, and a factor of two is one bit.  The same factor holds for the median and the 99 %
     quantile, which say more: the worst error is 5.8e-2 in both forms, at one point of skewness 700 where aluarw leaves the head
     both forms share with a relative error of 5e-11 and Phi's error-function bracket cancels to erfc(4) of its terms, so at the
     maximum the bound compares the shared head with itself.  flagrein: both forms and the truth agree at every point.  Points
     whose true ||d| - 6| < 1e-6 are not compared and must be fewer than 0.1 % of the draw.  ath is compared where the truth
     does not raise flagrein: the loop discards it otherwise.
  2. NaN or infinite wp, and sigmaw = 0 with 1/sigmaw = inf, give a non-finite ath in both forms (the loop's Gaussian arm and
     its !isfinite test downstream rely on the class).
  3. The float instances are the parent's: the gas recipe of tests/test_cbl_folds.py at compute_real_bytes = 4, 6000 particles,
     nz = 3, one step, gives the same bytes with a library built with -DFPX_CBL_NORMALISED=0 as with the product library.
     (cbl0_library builds that tagged library once per module, next to the product one: about half a minute where it does not
     exist yet.)
"""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPTS, SEED = 20000, 20251
EDGE_BAND, MAX_REJECTED = 1e-6, 1e-3
COLS = ("wp", "z", "wt", "ih", "rhoaux", "sigmaw", "irw", "dsigmawdz", "tlw", "ldirect")


def draw(n, seed):
    """n x 10 array of the probe's inputs: what a fine sub-step of the loop hands to cbl()"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.0, 1.0, n)
    z[0:40], z[40:80], z[80:120] = 1e-12, 1.0 - 1e-12, 1.0          # the ends; z = 1 makes (1 - z)**0.5 zero
    sigmaw = np.exp(rng.uniform(np.log(0.05), np.log(3.0), n))
    irw = 1.0 / sigmaw
    wp = sigmaw * rng.uniform(-5.0, 5.0, n)
    far = rng.random(n) < 0.05                                       # far enough out for flagrein
    wp[far] = (sigmaw * rng.uniform(8.0, 30.0, n) * rng.choice([-1.0, 1.0], n))[far]
    tlw = np.exp(rng.uniform(np.log(30.0), np.log(3000.0), n))
    dsigmawdz = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.0, -2.0, n)
    rhoaux = -1e-4 * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, n))
    wt = rng.uniform(0.0, 30.0, n)
    wt[rng.random(n) < 0.02] = 0.0                                   # the only way to skew == 0
    wt[100:110] = 0.0                                                # ... also at z = 1
    ih = 1.0 / rng.uniform(200.0, 3000.0, n)
    ldirect = rng.choice([-1.0, 1.0], n)
    return np.stack([wp, z, wt, ih, rhoaux, sigmaw, irw, dsigmawdz, tlw, ldirect], axis=1)


def probe(form, x):
    from flexpart_amd import _lib
    return _lib.cbl_probe(form, x)


@functools.lru_cache(maxsize=None)
def points_and_truth():
    x = draw(NPTS, SEED)
    x.setflags(write=False)
    t = np.load(os.path.join(ROOT, "tests", "golden", "cbl_truth_50digits.npz"))
    assert int(t["npts"]) == NPTS and int(t["seed"]) == SEED
    assert hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest() == t["inputs_sha256"].tobytes(), "the draw is not the one the truth was recorded for"
    return x, {k: t[k] for k in ("ath_hi", "ath_lo", "scale", "flagrein", "da", "db")}


def test_the_truth_belongs_to_the_draw():
    x, t = points_and_truth()
    assert all(len(v) == len(x) for v in t.values())
    edge = np.minimum(np.abs(np.abs(t["da"]) - 6.0), np.abs(np.abs(t["db"]) - 6.0)) < EDGE_BAND
    assert edge.mean() < MAX_REJECTED
    # the flag is the one the recorded d gives, and ath has a scale wherever the flag is down
    assert np.array_equal(t["flagrein"] == 1, (np.abs(t["da"]) > 6.0) & (np.abs(t["db"]) > 6.0))
    assert (t["scale"][t["flagrein"] == 0] > 0).all() and (np.abs(t["ath_lo"]) <= 2.0 ** -52 * np.abs(t["ath_hi"])).all()
    assert 50 < t["flagrein"].sum() < 0.5 * len(x)


def test_the_draw_covers_what_the_loop_hands_over():
    x = draw(NPTS, SEED)
    c = {k: x[:, j] for j, k in enumerate(COLS)}
    assert (c["z"] == 1.0).sum() >= 40 and (c["z"] == 1e-12).sum() == 40 and (c["z"] == 1.0 - 1e-12).sum() == 40
    assert c["z"].min() > 0.0 and c["z"].max() == 1.0
    assert 0.05 <= c["sigmaw"].min() < 0.06 and 2.9 < c["sigmaw"].max() <= 3.0 and np.all(c["irw"] == 1.0 / c["sigmaw"])
    assert 30.0 <= c["tlw"].min() and c["tlw"].max() <= 3000.0
    assert (c["dsigmawdz"] > 0).any() and (c["dsigmawdz"] < 0).any()
    assert np.all(np.abs(c["rhoaux"] + 1e-4) <= 1.0001e-5)
    assert (c["wt"] == 0.0).sum() > 100 and c["wt"].max() > 29.0
    assert set(np.unique(c["ldirect"])) == {-1.0, 1.0}
    near = np.abs(c["wp"]) <= 5.0 * c["sigmaw"]
    assert 0.9 < near.mean() < 0.97


@pytest.mark.gpu
def test_probe_against_truth(built):
    import mpmath as mp
    x, t = points_and_truth()
    edge = np.minimum(np.abs(np.abs(t["da"]) - 6.0), np.abs(np.abs(t["db"]) - 6.0)) < EDGE_BAND
    print(f"points on the edge of the flag's test, not compared: {int(edge.sum())} of {len(x)}")
    assert edge.mean() < MAX_REJECTED
    keep = ~edge
    use = np.flatnonzero(keep & (t["flagrein"] == 0))
    with mp.workdps(50):
        bth = [mp.mpf(float(sw)) * mp.sqrt(2 / mp.mpf(float(tl))) for sw, tl in zip(x[:, 5], x[:, 8])]
        ath = {i: mp.mpf(float(t["ath_hi"][i])) + mp.mpf(float(t["ath_lo"][i])) for i in use}
    stats = {}
    for form in (0, 1):
        got = probe(form, x)
        bad = np.flatnonzero(keep & (got[:, 2] != t["flagrein"]))
        assert bad.size == 0, (form, bad[:10])
        assert np.isfinite(got[use, 0]).all() and np.isfinite(got[:, 1]).all(), form
        with mp.workdps(50):
            eb = max(float(abs(mp.mpf(float(got[i, 1])) - bth[i]) / bth[i]) for i in np.flatnonzero(keep))
            ea = np.array([float(abs(mp.mpf(float(got[i, 0])) - ath[i]) / mp.mpf(float(t["scale"][i]))) for i in use])
        i = use[int(ea.argmax())]
        stats[form] = {"worst": float(ea.max()), "q99": float(np.quantile(ea, 0.99)), "median": float(np.median(ea)), "bth": eb}
        print(f"form {form}: error of ath in units of (|Phi| + |w2tl Q|)/ptot: worst {ea.max():.3e} (point {i}: {dict(zip(COLS, x[i]))}), "
              f"99 % {stats[form]['q99']:.3e}, median {stats[form]['median']:.3e}; of bth {eb:.3e}; {len(use)} points")
    for k in ("worst", "q99", "median", "bth"):
        assert stats[1][k] <= 2.0 * stats[0][k], (k, stats)


@pytest.mark.gpu
def test_special_inputs_keep_their_class(built):
    base = dict(wp=0.3, z=0.4, wt=8.0, ih=1.0 / 1200.0, rhoaux=-1e-4, sigmaw=0.9, irw=1.0 / 0.9, dsigmawdz=1e-3, tlw=200.0, ldirect=1.0)
    rows = []
    for wp in (np.nan, np.inf, -np.inf):
        for ldirect in (1.0, -1.0):
            rows.append(dict(base, wp=wp, ldirect=ldirect))
    for wp in (0.3, -0.3, 0.0):
        rows.append(dict(base, wp=wp, sigmaw=0.0, irw=np.inf))
    rows.append(dict(base))                                           # and an ordinary point, which must stay finite
    x = np.array([[r[k] for k in COLS] for r in rows])
    for form in (0, 1):
        ath = probe(form, x)[:, 0]
        print(form, ath)
        assert not np.isfinite(ath[:-1]).any(), (form, ath)
        assert np.isfinite(ath[-1])


FLOAT_RUN = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from flexpart_amd import synthetic as syn
from flexpart_amd.engine import Engine, RNG_TABLE_SEQ
from test_oracle_cpu import CASES
sc = syn.small(n=6000, nx=48, ny=32, nz=3, nsteps=1, ldirect=1, **dict(CASES["cbl"], ifine=11))
assert int(sc["cblflag"]) == 1
eng = Engine(sc, compute_real_bytes=4, host_real_bytes=4, rng_mode=RNG_TABLE_SEQ)
got = eng.run()[-1]
eng.close()
np.savez(sys.argv[2], **{k: np.asarray(v) for k, v in got.items()})
"""


@pytest.fixture(scope="module")
def cbl0_library(built):
    """the library with the dimensional body in every instance: the A/B partner of the product build"""
    import __graft_entry__ as g
    return g.build_library(extra_flags=["-DFPX_CBL_NORMALISED=0"], tag="cbl0")


@pytest.mark.gpu
def test_the_float_instance_is_the_parents(cbl0_library, tmp_path):
    variant = cbl0_library
    outs = []
    for name, lib in (("product", None), ("cbl0", variant)):
        env = {k: v for k, v in os.environ.items() if k != "FPX_LIBRARY"}
        if lib:
            env["FPX_LIBRARY"] = lib
        out = str(tmp_path / f"{name}.npz")
        subprocess.run([sys.executable, "-c", FLOAT_RUN, ROOT, out], check=True, env=env, timeout=300)
        outs.append(np.load(out))
    a, b = outs
    assert sorted(a.files) == sorted(b.files) and "ztra1" in a.files
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert (a["ztra1"] != 0).any()
