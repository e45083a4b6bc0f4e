"""Plume trajectories and their clustering on the device (iout = 4, 5): fpx_plumetraj_init, fpx_plumetraj, fpx_get_plumetraj,
fpx_plumetraj_time.  Reference: plumetraj.f90:56-230 (called at timemanager.f90:438) with clustering.f90, centerofmass.f90,
distance.f90, distance2.f90 and mean of mean_mod.

CPU: the numpy restatement tests/plumetraj_ref.py and the host-compiled device body (tests/plumetraj_host.cpp around
flexpart_amd/csrc/fpx_plumetraj.hpp) against what flang builds of the unmodified routines append to trajectories.txt
(tests/golden/pt_r4.npz, pt_r8.npz), byte for byte; the coverage of the cases; and the margins of every discrete decision
against the bounds of DESIGN section 21, which is what keeps the GPU comparison from being vacuous.
GPU: the kernels against the restatement applied to the downloaded particles.

A release point with fewer particles than clusters: clustering.f90:52 returns at once and the reference prints what its
locals held in rms, zrms and the cluster columns; the engine and the restatement write zeros there and no test compares
those columns of such a record (plumetraj_ref.defined_columns).

THE RULE of the GPU comparison.  Record count, jpoint, npart, the passes of the loop, numb, the three fractions and fclust are
EQUAL.  Every other value lies within plumetraj_ref.column_bounds of the restatement's, a bound computed from the
restatement's own statistics: (a) the reference's own serial summation error against the exactly rounded sum of the same
terms, plus the device's fp64 partials and one rounding; (b) 4 eps_H between the device's and the C library's sin, cos,
atan2 (8 x 2^-52 for the double functions inside distance and distance2), the figures DESIGN section 19 uses; (c) acos near
1, rerth dcrd / sin(angle); (d) first-order propagation through atan2, sqrt and mean's xq - xl^2/n.  The equalities hold
because every discrete decision of the cases used on the GPU ('blobs' in r4 and r8, 'diffuse' in r8) keeps a margin of at
least 1000 times the bound of what it compares (test_margins); 'diffuse' in r4 does not -- a wide cloud's bisectors lie
within the reference's own float summation error -- and is not run on the GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import plumetraj_ref as ref
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ("r4", "r8")
GPU_CASES = [("blobs", 8, 8), ("blobs", 4, 4), ("diffuse", 8, 8)]       # variant, compute_real_bytes, host_real_bytes
FACTOR = 1000.0
sys.path.insert(0, GOLD)


def kind_of(hb):
    return "r4" if hb == 4 else "r8"


@pytest.fixture(scope="module")
def restated():
    """The restatement of every (kind, variant) with its statistics: computed once, never modified."""
    out = {}
    for kind in KINDS:
        for v in syn.PT_VARIANTS:
            c = syn.plumetraj_case(v)
            st = ref.new_stats()
            out[kind, v] = (ref.run(c, kind, int(c["itime"]), stats=st), st)
    return out


def same_defined_bytes(got, want, recs, label=""):
    """Two files of records are equal in every column the reference defines."""
    g, w = got.decode().splitlines(), want.decode().splitlines()
    assert len(g) == len(w) == len(recs), (label, len(g), len(w), len(recs))
    for a, b, r in zip(g, w, recs):
        assert len(a) == len(b) == 306, (label, len(a), len(b))
        for lo, hi in ref.defined_columns(r):
            assert a[lo:hi] == b[lo:hi], (label, r["j"], lo, a[lo:hi], b[lo:hi])


# ---- CPU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", syn.PT_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(restated, kind, variant):
    gold = np.load(os.path.join(GOLD, f"pt_{kind}.npz"))[f"records_{variant}"].tobytes()
    recs, _ = restated[kind, variant]
    same_defined_bytes(ref.text(recs).encode(), gold, recs, f"{kind} {variant}")
    assert [r["j"] for r in recs] == [1, 4, 5, 6, 7] and sum(r["clustered"] for r in recs) == 4
    # the age column: itime - (ireleasestart + ireleaseend) / 2 with Fortran's division (point 4: -5401 / 2 = -2700)
    assert [r["age"] for r in recs] == [900, 2700, -450, 5400, 4050]


@pytest.mark.ref
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_a_live_build_of_the_reference(kind, tmp_path):
    import make_plumetraj_golden as mk
    if not mk.available():
        pytest.skip("flang or the reference tree is not present")
    exe = mk.build(kind, str(tmp_path))
    for v in syn.PT_VARIANTS:
        c = syn.plumetraj_case(v)
        recs = ref.run(c, kind, int(c["itime"]))
        same_defined_bytes(ref.text(recs).encode(), mk.run(exe, c, int(c["itime"]), str(tmp_path)), recs, f"live {kind} {v}")


@pytest.fixture(scope="module")
def host_body(tmp_path_factory):
    d = tmp_path_factory.mktemp("pt_host")
    exe = d / "plumetraj_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(HERE, "plumetraj_host.cpp"), "-o", str(exe)])
    return str(exe), d


def host_input(c, kind, itime, path):
    """The input of tests/plumetraj_host.cpp: per active release point with particles its positions and the interpolated
    topo, pvi, hmixi, tri of partavg_ref.addends."""
    rt = ref.RT[kind]
    P = ref.pr.Params(c, kind)
    lage = int(np.asarray(c["lage"]).ravel()[-1])
    blocks = []
    for j, (s, e) in enumerate(zip(c["ireleasestart"], c["ireleaseend"]), 1):
        who = np.nonzero((np.asarray(c["itra1"]) == itime) & (np.asarray(c["npoint"]) == j))[0]
        if abs(int(s) - itime) > lage or who.size == 0:
            continue
        xt, yt, zt = np.asarray(c["xtra1"])[who], np.asarray(c["ytra1"])[who], np.asarray(c["ztra1"])[who].astype(rt)
        a = ref.pr.addends(P, itime, xt, yt, zt)
        blocks.append((np.array([j, itime - int((int(s) + int(e)) / 2), who.size], np.int32), xt, yt, zt, a["topo"], a["pv"], a["hmix"], a["tro"]))
    with open(path, "wb") as f:
        np.array([4 if kind == "r4" else 8, ref.NCLUSTER, len(blocks)], np.int32).tofile(f)
        g = c["geom"]
        np.array([g[2], g[3], g[0], g[1]], np.float64).tofile(f)
        for b in blocks:
            b[0].tofile(f)
            np.asarray(b[1], np.float64).tofile(f); np.asarray(b[2], np.float64).tofile(f)
            for a in b[3:]:
                np.asarray(a).astype(rt).tofile(f)


@pytest.mark.parametrize("variant", syn.PT_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_compiled_device_body_reproduces_the_reference(host_body, restated, kind, variant):
    """The per-particle terms, the per-release-point formulas, the decisions and the formatter of fpx_plumetraj.hpp, compiled
    as host code and run serially in storage order with accumulators of the host's real kind, give the reference's records
    byte for byte, and the restatement's passes and numb."""
    exe, d = host_body
    c = syn.plumetraj_case(variant)
    fin = str(d / f"in_{kind}_{variant}.bin")
    host_input(c, kind, int(c["itime"]), fin)
    out = subprocess.check_output([exe, fin])
    lines = out.decode().splitlines()
    recs, _ = restated[kind, variant]
    gold = np.load(os.path.join(GOLD, f"pt_{kind}.npz"))[f"records_{variant}"].tobytes()
    same_defined_bytes(("\n".join(lines[0::2]) + "\n").encode(), gold, recs, f"host {kind} {variant}")
    for line, r in zip(lines[1::2], recs):
        got = [int(t) for t in line[1:].split()]
        assert got == [r["passes"]] + [int(q) for q in r["numb"]], (r["j"], got)


def test_formatter_edge_cases():
    """Fw.d of the record: ties of the exact binary value go to even, f7.0 keeps its point, a value that does not fit drops the
    optional zero or prints asterisks, a negative value that rounds to zero keeps its sign."""
    assert ref.fmt_f(0.125, 8, 2) == "    0.12" and ref.fmt_f(0.375, 8, 2) == "    0.38"
    assert ref.fmt_f(2.5, 7, 0) == "     2." and ref.fmt_f(3.5, 7, 0) == "     4."
    assert ref.fmt_f(-0.04, 6, 1) == "  -0.0" and ref.fmt_f(123456.7, 6, 1) == "******"
    assert ref.fmt_f(-0.5, 4, 2) == "-.50" and ref.fmt_i(123456, 5) == "*****"


def test_cases_cover_every_branch(restated):
    """Everything the routines can do appears in the cases the GPU test uses, counted by the restatement while it runs."""
    used = [(kind_of(hb), v) for v, _, hb in GPU_CASES]
    passes, exits = set(), set()
    empty_cluster = chunks = 0
    for key in used:
        recs, st = restated[key]
        assert st["inactive"] == 1 and st["empty"] == 1 and st["few"] == 1, st          # point 2, point 3, point 4
        assert st["guard"] == 0                                                         # no particle needs a guard
        assert st["pv_north"] > 100 and st["pv_south"] > 100                            # both signs of yl in the PV test
        assert st["in_box2"] > 0 and st["in_box"] > 0                                   # a pair inside each distance box
        empty_cluster += st["empty_cluster"]
        for r in recs:
            if r["clustered"]:
                passes.add(r["passes"])
            chunks = max(chunks, -(-r["n"] // 1024))
            assert r["n"] != 5 or (r["passes"] == 100 and list(r["numb"]) == [1] * 5)
        for p in st["points"].values():
            exits |= {e[0] for e in p["exit"]}
        # both sides of hmix, of the tropopause and of |PV| = 2 in the large point
        v = recs[0]["values"]
        assert all(0.0 < v[k] < 100.0 for k in (11, 12, 13)), v[11:14]
    assert empty_cluster > 0 and chunks == 3
    assert 2 in passes and max(passes - {100}) >= 4 and 100 in passes
    assert exits == {"soft", "exact", "nan"}


@pytest.mark.parametrize("variant,kind", [(v, kind_of(hb)) for v, _, hb in GPU_CASES])
def test_margins(restated, variant, kind):
    """The condition that keeps the GPU test from being vacuous: every decision of the restatement -- nearest against
    second-nearest centroid, the exit test, the two boxes -- keeps a margin of at least 1000 times the bound of the
    quantities it compares, concluded from the restatement alone.  An exit whose ratio is exactly 0 because the centroids
    repeat bitwise, or 0/0 because every distance is exactly 0, has no bound to keep: the assignments and the box decisions
    behind it are covered by theirs."""
    recs, st = restated[kind, variant]
    worst = {}
    for j, p in st["points"].items():
        items = [("gap", m, b) for m, b in p["gap"]] + [("box2", m, b) for m, b in p["box2"]] + [("box",) + tuple(p["box"])]
        items += [("exit", m, b) for what, m, b in p["exit"] if what == "soft"]
        for name, m, b in items:
            if b > 0:
                worst[name] = min(worst.get(name, np.inf), m / b)
            assert m >= FACTOR * b, (variant, kind, j, name, m, b)
    print(f"{variant} [{kind}] smallest margin / bound:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_diffuse_in_r4_is_legitimately_ill_conditioned(restated):
    """Why 'diffuse' runs on the GPU in r8 only: in r4 its smallest gap between two centroids is within the factor of the bound."""
    _, st = restated["r4", "diffuse"]
    assert min(m / b for p in st["points"].values() for m, b in p["gap"] if b > 0) < FACTOR


def test_column_bounds_are_small(restated):
    """A column whose bound exceeds 1 % of its value's scale would mean a badly chosen case."""
    for v, _, hb in GPU_CASES:
        kind = kind_of(hb)
        recs, st = restated[kind, v]
        vals = np.array([r["values"].astype(np.float64) for r in recs])
        scale = np.abs(vals).max(axis=0)
        for r in recs:
            b = ref.column_bounds(r, st["points"][r["j"]], kind)
            ok = ~np.isnan(b) & (scale > 0)
            assert (b[ok] <= 0.01 * scale[ok]).all(), (v, kind, r["j"], np.nonzero(ok & (b > 0.01 * scale))[0])


def test_header_cites_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    for name in ("fpx_plumetraj_init", "fpx_get_plumetraj", "fpx_plumetraj_time", "FPX_MAXCLUSTER", "timemanager.f90:438", "plumetraj.f90:56-230",
                 "plumetraj.f90:218-225", "clustering.f90:52"):
        assert name in text, name


# ---- GPU ------------------------------------------------------------------------------------------------------

def make_engine(sc, cb, hb, **kw):
    from flexpart_amd.engine import Engine, RNG_PHILOX
    eng = Engine(sc, compute_real_bytes=cb, host_real_bytes=hb, rng_mode=RNG_PHILOX, seed=4711, **kw)
    eng.upload_diag_fields_from_scenario(sc)
    return eng


def downloaded(sc, eng):
    d = eng.download()
    src = dict(sc)
    src.update({k: d[k] for k in ("xtra1", "ytra1", "ztra1", "itra1", "npoint")})
    return src


def compare_records(got, recs, st, kind, label):
    """THE RULE of the module's docstring; prints the largest difference in units of its bound."""
    assert list(got["jpoint"]) == [r["j"] for r in recs], label
    assert list(got["npart"]) == [r["n"] for r in recs], label
    assert list(got["iterations"]) == [r["passes"] for r in recs], (label, got["iterations"])
    worst = 0.0
    for i, r in enumerate(recs):
        if r["clustered"]:
            assert list(got["numb"][i]) == [int(q) for q in r["numb"]], (label, r["j"])
        b = ref.column_bounds(r, st["points"][r["j"]], kind)
        g, w = got["values"][i].astype(np.float64), r["values"].astype(np.float64)
        for k in range(b.size):
            if np.isnan(b[k]):
                continue
            if b[k] == 0:
                assert g[k] == w[k], (label, r["j"], k, g[k], w[k])
            else:
                worst = max(worst, abs(g[k] - w[k]) / b[k])
                assert abs(g[k] - w[k]) <= b[k], (label, r["j"], k, g[k], w[k], b[k])
    print(f"{label}: largest |difference| / bound = {worst:.3g}")


def compare_file(data, recs, st, kind, label):
    """Same line count, integer columns equal, every fixed-point column within its bound plus half a unit of its last place."""
    lines = data.decode().splitlines()
    assert len(lines) == len(recs), label
    widths = [5, 8] + [w for w, _ in ref.FMT] + [w for w, _ in ref.CFMT] * ref.NCLUSTER
    places = [d for _, d in ref.FMT] + [d for _, d in ref.CFMT] * ref.NCLUSTER
    pos = np.concatenate([[0], np.cumsum(widths)])
    for line, r in zip(lines, recs):
        assert len(line) == pos[-1]
        assert int(line[0:5]) == r["j"] and int(line[5:13]) == r["age"], (label, line[:13])
        b = ref.column_bounds(r, st["points"][r["j"]], kind)
        for k in range(b.size):
            if np.isnan(b[k]):
                continue
            v = float(line[pos[k + 2]:pos[k + 3]])
            assert abs(v - float(r["values"][k])) <= b[k] + 0.5 * 10.0 ** -places[k] + 1e-12, (label, r["j"], k, v, r["values"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("variant,cb,hb", GPU_CASES)
def test_kernels_against_the_restatement(built, tmp_path, variant, cb, hb):
    """Straight after the upload and after one step: the records and the appended file against the restatement applied to the
    downloaded particles.  Fails on an engine without the feature: the symbols do not exist."""
    kind = kind_of(hb)
    sc = syn.plumetraj_case(variant)
    eng = make_engine(sc, cb, hb)
    eng.plumetraj_init(sc["ireleasestart"], sc["ireleaseend"])
    path = str(tmp_path / "trajectories.txt")
    open(path, "w").write("header\n")
    size = len("header\n")
    for phase in ("upload", "step"):
        if phase == "step":
            eng.step()
        src = downloaded(sc, eng)
        st = ref.new_stats()
        recs = ref.run(src, kind, eng.itime, stats=st)
        nrec = eng.plumetraj(eng.itime, path)
        assert nrec == len(recs) == 5
        compare_records(eng.get_plumetraj(), recs, st, kind, f"{variant} [{kind}] {phase}")
        data = open(path, "rb").read()
        compare_file(data[size:], recs, st, kind, f"{variant} [{kind}] {phase} file")     # appended behind what the host wrote
        size = len(data)
        assert eng.plumetraj_time() > 0
    assert data.startswith(b"header\n")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cb,hb", [(8, 8), (4, 4)])
def test_reproducibility(built, cb, hb):
    """Two calls on the same state give the same bits; so does a call after fpx_sort_particles (the list is laid out by
    particle number, which a locality sort does not change) and an engine with four times the storage spaces."""
    sc = syn.plumetraj_case("diffuse")
    eng = make_engine(sc, cb, hb)
    eng.plumetraj_init(sc["ireleasestart"], sc["ireleaseend"])
    eng.step()
    eng.plumetraj()
    a = eng.get_plumetraj()
    eng.plumetraj()
    b = eng.get_plumetraj()
    eng.sort()
    eng.plumetraj()
    c = eng.get_plumetraj()
    eng.close()
    big = make_engine(sc, cb, hb, max_particles=4 * int(sc["npart"]))
    big.plumetraj_init(sc["ireleasestart"], sc["ireleaseend"])
    big.step()
    big.plumetraj()
    d = big.get_plumetraj()
    big.close()
    assert len(a["jpoint"]) == 5 and a["iterations"].max() == 100
    for other in (b, c, d):
        for k in a:
            assert a[k].tobytes() == other[k].tobytes(), k


@pytest.mark.gpu
def test_states_and_refusals(built, tmp_path):
    from flexpart_amd import _lib
    from flexpart_amd.engine import Engine, _vp
    sc = syn.plumetraj_case("blobs")
    eng = make_engine(sc, 8, 8)
    lib = eng.lib
    assert lib.fpx_plumetraj(eng.h, 0, None, None) == -3 and b"fpx_plumetraj_init first" in lib.fpx_last_error()
    assert lib.fpx_get_plumetraj(eng.h, 7, None, None, None, None, None, 39) == -3
    a = np.ascontiguousarray(sc["ireleasestart"], np.int32); b = np.ascontiguousarray(sc["ireleaseend"], np.int32)
    for k in (0, 9):
        cfg = _lib.FpxPlumetrajCfg(C.sizeof(_lib.FpxPlumetrajCfg), a.size, k, 0, a.ctypes.data, b.ctypes.data)
        assert lib.fpx_plumetraj_init(eng.h, C.byref(cfg)) == -1 and b"ncluster" in lib.fpx_last_error()
    eng.plumetraj_init(a, b, ncluster=4)
    assert lib.fpx_plumetraj(eng.h, 0, str(tmp_path / "t.txt").encode(), None) == -1 and b"five clusters" in lib.fpx_last_error()
    assert eng.plumetraj(0) == 5                                      # without a path any ncluster runs
    assert eng.get_plumetraj()["values"].shape == (5, 34)
    v = np.zeros((7, 33))
    assert lib.fpx_get_plumetraj(eng.h, 7, None, None, None, None, _vp(v), 33) == -1 and b"ld" in lib.fpx_last_error()
    assert lib.fpx_get_plumetraj(eng.h, 4, None, None, None, None, None, 34) == -1
    eng.close()
    bare = {k: v for k, v in sc.items() if k not in ("uu", "vv", "ww")}
    eng = Engine(bare, compute_real_bytes=8, host_real_bytes=8)       # no wind fields: the slots are not loaded
    eng.plumetraj_init(a, b)
    assert lib.fpx_plumetraj(eng.h, 0, None, None) == -3
    eng.close()
    eng = make_engine(sc, 8, 8)                                       # a two-rank host communicator
    eng.plumetraj_init(a, b)
    cb = _lib.ALLREDUCE_FN(lambda user, send, recv, count, dtype: 0)
    assert lib.fpx_comm_init_host(eng.h, 2, 0, cb, None) == 0
    assert lib.fpx_plumetraj(eng.h, 0, None, None) == -5 and b"several ranks" in lib.fpx_last_error()
    eng.close()


@pytest.mark.gpu
def test_the_feature_changes_nothing_else(built):
    """A step gives the same particles bit for bit on a handle that initialised the feature (and called it) and on one that never did."""
    sc = syn.plumetraj_case("diffuse")
    res = []
    for on in (False, True):
        eng = make_engine(sc, 8, 8)
        if on:
            eng.plumetraj_init(sc["ireleasestart"], sc["ireleaseend"])
            eng.plumetraj()
        eng.step()
        res.append(eng.download())
        eng.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k
