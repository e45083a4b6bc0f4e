"""Boundary conditions of a domain-filling run on the device (mdomainfill = 1, 2): fpx_domainfill_init,
fpx_boundcond_domainfill, fpx_get/set_domainfill_acc, fpx_boundcond_output, fpx_domainfill_time.  Reference:
boundcond_domainfill.f90:54-573 (called every time step at timemanager.f90:240) with ran1, random_mod.f90:12-42.

CPU: the numpy restatement tests/domainfill_ref.py and the host-compiled device bodies (tests/domainfill_host.cpp around
flexpart_amd/csrc/fpx_domainfill.hpp, run in the stages of the device call) against what flang builds of the unmodified
routine leave behind after each of four consecutive calls (tests/golden/bc_r4.npz, bc_r8.npz), and the branch coverage of
the cases.  GPU: the C ABI against the same fixtures.

THE RULE of every comparison with the reference: itra1 of all storage spaces, numpart, numparticlecount, acc_mass_we and
acc_mass_sn bit for bit; every particle array of the spaces with itra1 = itime bit for bit; boundcond.bin byte for byte.
The positions of the spaces with itra1 /= itime are not compared: the reference leaves a rejected candidate's coordinates
in the vacant space it looked at.

The refusals need a handle, and a handle needs a device: they are pinned in the GPU part."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import domainfill_ref as ref
from flexpart_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KINDS = ("r4", "r8")
RUNNING = ("fill1", "fill2", "xglobal")                 # the variants whose four calls all succeed and change something
ARRAYS = ("itramem", "npoint", "nclass", "idt", "itrasplit", "xtra1", "ytra1", "ztra1", "xmass1")
sys.path.insert(0, GOLD)


def kind_of(hb):
    return "r4" if hb == 4 else "r8"


@pytest.fixture(scope="module")
def gold():
    return {k: np.load(os.path.join(GOLD, f"bc_{k}.npz")) for k in KINDS}


@pytest.fixture(scope="module")
def restated():
    """The restatement of every (kind, variant) with its branch counters: computed once, never modified."""
    out = {}
    for kind in KINDS:
        for v in syn.DF_VARIANTS:
            st = ref.new_stats()
            out[kind, v] = (ref.run(syn.domainfill_case(v), kind, syn.DF_CALLS, st), st)
    return out


def same_as_reference(state, g, v, i, itime, kind, label):
    """THE RULE of the module's docstring for the state after call i (0-based)."""
    rt = ref.RT[kind]
    key = lambda k: g[f"{v}_{i}_{k}"]
    assert int(state["numpart"]) == int(key("numpart")), (label, i, "numpart", state["numpart"], int(key("numpart")))
    assert int(state["numparticlecount"]) == int(key("numparticlecount")), (label, i, "numparticlecount")
    assert np.array_equal(np.asarray(state["itra1"], np.int32), key("itra1")), (label, i, "itra1", np.nonzero(np.asarray(state["itra1"]) != key("itra1"))[0])
    for k in ("acc_mass_we", "acc_mass_sn"):
        assert np.asarray(state[k]).astype(rt).tobytes() == key(k).tobytes(), (label, i, k)
    live = key("itra1") == itime
    assert live.sum() > 100
    for k in ARRAYS:
        a = np.asarray(state[k])
        a = a.reshape(-1, a.shape[-1])[0]
        want = key(k)
        got = a.astype(want.dtype)
        assert got[live].tobytes() == want[live].tobytes(), (label, i, k, np.nonzero(live & (got != want))[0][:5])


# ---- CPU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", syn.DF_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_reproduces_the_reference(restated, gold, kind, variant):
    g = gold[kind]
    out, _ = restated[kind, variant]
    status, ncalls = (int(x) for x in g[f"{variant}_status"])
    if variant == "full":                                # the reference stops in the first call (stop 1, :307-310)
        assert (status, ncalls) == (1, 0) and out == [(None, None)]
        return
    assert (status, ncalls) == (0, syn.DF_CALLS) and len(out) == syn.DF_CALLS
    c = syn.domainfill_case(variant)
    itime = int(c["itime"])
    nxmax, nymax, maxcolumn = (int(x) for x in g["par"])
    for i, (s, r) in enumerate(out):
        if variant == "gdomainfill":
            assert r["n_released"] == r["n_terminated"] == 0
            first = ref.initial_state(c, kind)
            for k in ARRAYS + ("acc_mass_we", "acc_mass_sn"):          # itra1 moves on between the calls, nothing else changes
                assert np.asarray(g[f"{variant}_{i}_{k}"]).tobytes() == np.asarray(first[k]).tobytes(), k
        else:
            same_as_reference(s, g, variant, i, itime, kind, f"restatement {kind} {variant}")
        itime += int(c["lsynctime"])
    if variant in RUNNING:
        assert ref.boundcond_bin(c, out[-1][0], kind, nxmax, nymax, maxcolumn) == g[f"{variant}_bin"].tobytes()
        assert sum(r["n_released"] + r["n_rejected"] for _, r in out) > 20 and out[0][1]["n_terminated"] >= 3


@pytest.mark.ref
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_matches_a_live_build_of_the_reference(kind, tmp_path):
    import make_domainfill_golden as mk
    if not mk.available():
        pytest.skip("flang or the reference tree is not present")
    exe = mk.build(kind, str(tmp_path))
    for v in ("fill2", "full"):
        c = syn.domainfill_case(v)
        calls, rc, _ = mk.run(exe, c, kind, syn.DF_CALLS, str(tmp_path))
        out = ref.run(c, kind, syn.DF_CALLS)
        assert (rc, len(calls)) == ((1, 0) if v == "full" else (0, syn.DF_CALLS))
        for i, r in enumerate(calls):
            assert np.array_equal(out[i][0]["itra1"], r["itra1"]) and out[i][0]["acc_mass_we"].tobytes() == r["acc_mass_we"].tobytes()


@pytest.fixture(scope="module")
def host_body(tmp_path_factory):
    d = tmp_path_factory.mktemp("df_host")
    exe = d / "domainfill_host"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(HERE, "domainfill_host.cpp"), "-o", str(exe)])
    return str(exe), d


@pytest.mark.parametrize("variant", syn.DF_VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_compiled_device_body_reproduces_the_reference(host_body, gold, kind, variant):
    """df_flux, df_candidate and df_nclass of fpx_domainfill.hpp as host code, run in the stages of the device call (flags,
    flux of every location, scan, candidates with their places in the serial stream, scan of the accepted, k-th accepted into
    the k-th vacancy, all or nothing), leave what the reference leaves."""
    import make_domainfill_golden as mk
    exe, d = host_body
    g = gold[kind]
    c = syn.domainfill_case(variant)
    fin, fout = str(d / f"in_{kind}_{variant}.bin"), str(d / f"out_{kind}_{variant}.bin")
    mk.write_input(c, syn.DF_CALLS, fin + ".body")
    with open(fin, "wb") as f:
        np.array([4 if kind == "r4" else 8], np.int32).tofile(f)
        f.write(open(fin + ".body", "rb").read())
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    calls = mk.read_output(c, kind, fout)
    if variant == "full":
        assert p.returncode == 1 and calls == [] and p.stdout.startswith("stopped 0")
        return
    assert p.returncode == 0 and len(calls) == syn.DF_CALLS, p.stderr
    itime = int(c["itime"])
    for i, r in enumerate(calls):
        if variant != "gdomainfill":
            same_as_reference(r, g, variant, i, itime, kind, f"host {kind} {variant}")
        else:
            assert all(np.asarray(r[k]).tobytes() == np.asarray(g[f"{variant}_{i}_{k}"]).tobytes() for k in r)
        itime += int(c["lsynctime"])
    if variant != "gdomainfill":
        b = [int(t) for t in p.stdout.split()[1:]]       # B_DZ_FIRST, B_DZ_LAST, B_DZ_MID, B_CORNER, B_IN, B_OUT, B_MM2
        assert len(b) == 7 and all(x > 0 for x in b[:6]), b


def test_cases_cover_every_branch(restated):
    """Everything the routine can do appears in the cases the GPU tests run, counted by the restatement while it runs: the
    three deltaz and the three ztra1 cases, corner rows, both outcomes of the sign rule on each of the four sides, a location
    that releases two particles in one call, both reasons of rejection, the sign flip of the southern hemisphere, and
    terminations through either test."""
    for kind in KINDS:
        _, st = restated[kind, "fill2"]
        assert all(st[b] > 0 for b in ref.BRANCHES), {b: st[b] for b in ref.BRANCHES if st[b] == 0}
        _, st = restated[kind, "fill1"]
        assert all(st[b] > 0 for b in ref.BRANCHES if not b.startswith("rejected")), st
        assert st["rejected_low"] == st["rejected_pv"] == 0
        _, st = restated[kind, "xglobal"]
        assert st["terminated_x"] == 0 and st["terminated_y"] > 0 and st["accepted"] > 20
        out, _ = restated[kind, "fill2"]
        assert all(r["n_rejected"] > 0 for _, r in out) and sum(r["n_released"] for _, r in out) >= 5
        out, _ = restated[kind, "fill1"]
        assert max(s["numpart"] for s, _ in out) > int(syn.domainfill_case("fill1")["numpart"])      # :303 raises numpart
    c = syn.domainfill_case("fill1")
    counts = set(int(v) for v in np.asarray(c["numcolumn_we"])[1:9].ravel()) | set(int(v) for v in np.asarray(c["numcolumn_sn"])[2:10].ravel())
    assert counts == {0, 1, 3, 4, 6}


def test_abi_is_unchanged_and_the_new_structs_match(tmp_path):
    """fpx_abi_version() == 4, sizeof(fpx_config) equals the ctypes mirror, and so do the two new structs."""
    from flexpart_amd import _lib
    pairs = [("fpx_config", _lib.FpxConfig), ("fpx_domainfill_cfg", _lib.FpxDomainfillCfg), ("fpx_domainfill_stats", _lib.FpxDomainfillStats),
             ("fpx_plumetraj_cfg", _lib.FpxPlumetrajCfg)]
    src = tmp_path / "sizes.c"
    src.write_text('#include "flexpart_amd.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) {\n'
                   + "".join(f'  printf("{n} %zu\\n", sizeof({n}));\n' for n, _ in pairs)
                   + '  printf("off %zu\\n", offsetof(fpx_config, device_initcond));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n, t in pairs:
        assert int(got[n]) == C.sizeof(t), (n, got[n], C.sizeof(t))
    assert int(got["off"]) == _lib.FpxConfig.device_initcond.offset


def test_library_exports_the_new_symbols(built):
    from flexpart_amd import _lib
    lib = _lib.load()
    assert lib.fpx_abi_version() == 4
    for n in ("fpx_domainfill_init", "fpx_boundcond_domainfill", "fpx_get_domainfill_acc", "fpx_set_domainfill_acc", "fpx_boundcond_output",
              "fpx_domainfill_time"):
        assert hasattr(lib, n) and n in _lib.SYMBOLS, n
    assert lib.fpx_domainfill_init(None, None) == -1      # a null handle is refused before anything else


def test_header_cites_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "flexpart_amd.h")).read()
    for name in ("timemanager.f90:240", "boundcond_domainfill.f90:54-573", "random_mod.f90:12-42", ":307-310", ":568-572", "par_mod.f90:101"):
        assert name in text, name


# ---- GPU ------------------------------------------------------------------------------------------------------

def make_engine(sc, hb, rng=None, pad=(0, 0, 0), maxcolumn=None, init=True):
    from flexpart_amd.engine import Engine, RNG_TABLE_SEQ
    eng = Engine(sc, compute_real_bytes=hb, host_real_bytes=hb, rng_mode=RNG_TABLE_SEQ if rng is None else rng, seed=4711,
                 max_particles=int(sc["npart"]), pad=pad)
    eng.upload_diag_fields_from_scenario(sc)
    eng.set_numpart(int(sc["numpart"]))
    if init:
        eng.domainfill_init(sc, maxcolumn=maxcolumn)
    return eng


def device_state(eng, sc):
    nx, ny, _ = (int(v) for v in sc["grid"])
    d = eng.download(count=int(sc["npart"]))
    we, sn = eng.get_domainfill_acc(compact=(ny, nx, syn.DF_MAXCOLUMN))
    d.update(acc_mass_we=we, acc_mass_sn=sn, numpart=eng.n, numparticlecount=eng.numparticlecount)
    return d


def move_on(eng, sc, d, itime):
    """What the particle loop does to the time stamps between two calls, through the C ABI: the whole state goes back up."""
    up = {k: v for k, v in d.items() if k not in ("acc_mass_we", "acc_mass_sn", "numpart", "numparticlecount")}
    up["itra1"] = np.where(d["itra1"] == itime, itime + int(sc["lsynctime"]), d["itra1"]).astype(np.int32)
    up["npart"] = int(sc["npart"])
    n = eng.n
    eng.upload_particles_from_scenario(up)
    eng.n = n
    eng.set_numpart(n)


def same_bits(a, b, keys=None):
    for k in keys or a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("variant", RUNNING)
@pytest.mark.parametrize("hb", [4, 8])
def test_parity_mode_equals_the_reference(built, gold, restated, tmp_path, hb, variant, sort):
    """Through the C ABI with the serial ran1 stream: after each of the four calls the device holds what the reference holds
    (THE RULE), also with a locality sort between the calls; the statistics are the restatement's; boundcond.bin is the
    reference's byte for byte (the engine has par_mod's extents then).  Fails on an engine without the feature: the symbols
    do not exist."""
    kind = kind_of(hb)
    g = gold[kind]
    sc = syn.domainfill_case(variant)
    nxmax, nymax, maxcolumn = (int(x) for x in g["par"])
    nx, ny, _ = (int(v) for v in sc["grid"])
    eng = make_engine(sc, hb, pad=(0, 0, 0) if sort else (nxmax - nx, nymax - ny, 0), maxcolumn=None if sort else maxcolumn)
    out, _ = restated[kind, variant]
    itime = int(sc["itime"])
    for i in range(syn.DF_CALLS):
        if sort:
            eng.sort()
        st = eng.boundcond_domainfill(itime)
        d = device_state(eng, sc)
        same_as_reference(d, g, variant, i, itime, kind, f"device {kind} {variant} sort={sort}")
        r = out[i][1]
        assert (st["n_terminated"], st["n_released"], st["n_rejected"], st["numactiveparticles"]) == \
               (r["n_terminated"], r["n_released"], r["n_rejected"], r["numactiveparticles"]), (i, st)
        assert abs(st["accmasst"] - float(r["accmasst"])) <= 1e-5 * float(r["accmasst"])      # a sum of ~350 terms of one sign, r4 at worst
        assert eng.domainfill_time() > 0
        move_on(eng, sc, d, itime)
        itime += int(sc["lsynctime"])
    if not sort:
        path = str(tmp_path / "boundcond.bin")
        eng.boundcond_output(path)
        assert open(path, "rb").read() == g[f"{variant}_bin"].tobytes()
    eng.close()


@pytest.mark.gpu
def test_gdomainfill_touches_nothing(built):
    sc = syn.domainfill_case("gdomainfill")
    eng = make_engine(sc, 8)
    before = device_state(eng, sc)
    st = eng.boundcond_domainfill(0)
    after = device_state(eng, sc)
    same_bits(before, after)
    assert all(v == 0 for v in st.values())
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hb", [4, 8])
def test_full_returns_the_error_and_changes_nothing(built, hb):
    """More candidates than vacancies: FPX_ERR_NOMEM; particles, acc_mass, numpart, numparticlecount as before; and the stream
    too -- after room has been made the next call does what it does on a handle that never failed."""
    sc = syn.domainfill_case("full")
    res = []
    for fail_first in (True, False):
        eng = make_engine(sc, hb)
        before = device_state(eng, sc)
        if fail_first:
            n = C.c_int64(eng.n); npc = C.c_int32(eng.numparticlecount)
            rc = eng.lib.fpx_boundcond_domainfill(eng.h, 0, C.byref(n), C.byref(npc), None)
            assert rc == -4 and b"too many particles" in eng.lib.fpx_last_error()
            assert (n.value, npc.value) == (eng.n, eng.numparticlecount)
            same_bits(before, device_state(eng, sc))
        room = dict(before)
        room["itra1"] = np.where(np.arange(int(sc["npart"])) % 3 == 1, ref.DEAD, before["itra1"]).astype(np.int32)
        move_on(eng, sc, room, -1)
        st = eng.boundcond_domainfill(0)
        assert st["n_released"] > 10
        res.append(device_state(eng, sc))
        eng.close()
    same_bits(res[0], res[1])


@pytest.mark.gpu
@pytest.mark.parametrize("hb", [4, 8])
def test_counter_mode(built, gold, restated, hb):
    """Philox: terminations, mmass (through acc_mass and the counts), the storage spaces taken, npoint and the counts are those
    of the parity mode for fill1, where every candidate is accepted; the positions lie inside their cells and height
    ranges; two runs give the same bits, with and without a locality sort."""
    from flexpart_amd.engine import RNG_PHILOX
    kind = kind_of(hb)
    g = gold[kind]
    sc = syn.domainfill_case("fill1")
    out, _ = restated[kind, "fill1"]
    runs = []
    for sort in (False, False, True):
        eng = make_engine(sc, hb, rng=RNG_PHILOX)
        itime = int(sc["itime"])
        states = []
        for i in range(syn.DF_CALLS):
            if sort:
                eng.sort()
            st = eng.boundcond_domainfill(itime)
            d = device_state(eng, sc)
            states.append(d)
            r = out[i][1]
            assert (st["n_terminated"], st["n_released"], st["n_rejected"]) == (r["n_terminated"], r["n_released"], 0)
            key = lambda k: g[f"fill1_{i}_{k}"]
            assert np.array_equal(d["itra1"], key("itra1")) and (d["numpart"], d["numparticlecount"]) == (int(key("numpart")), int(key("numparticlecount")))
            for k in ("acc_mass_we", "acc_mass_sn"):
                assert d[k].tobytes() == key(k).tobytes(), k
            live = key("itra1") == itime
            for k in ("npoint", "itramem", "idt", "itrasplit", "nclass"):
                assert np.array_equal(d[k][live], key(k)[live]), k
            assert d["xmass1"][0][live].astype(key("xmass1").dtype).tobytes() == key("xmass1")[live].tobytes()
            for q in r["released"]:
                p, row = q["space"], q["row"]
                fixed, free = (d["xtra1"][p], d["ytra1"][p]) if q["side"] == "we" else (d["ytra1"][p], d["xtra1"][p])
                assert fixed == float((sc["nx_we"] if q["side"] == "we" else sc["ny_sn"])[q["k"]])
                lo, hi = {-1: (row, row + 0.5), 0: (row - 0.5, row + 0.5), 1: (row - 0.5, row)}[q["corner"]]
                assert lo <= free <= hi, (q, free)
                if q["zlo"] is None:
                    assert d["ztra1"][p] == float(key("ztra1")[p])               # no uniform in it
                else:
                    assert q["zlo"] <= d["ztra1"][p] <= q["zhi"], (q, d["ztra1"][p])
            move_on(eng, sc, d, itime)
            itime += int(sc["lsynctime"])
        eng.close()
        runs.append(states)
    for a, b in zip(runs[0], runs[1]):
        same_bits(a, b)
    for i, (a, b) in enumerate(zip(runs[0], runs[2])):                          # a locality sort leaves the vacant spaces behind numpart
        same_bits(a, b, ("itra1", "acc_mass_we", "acc_mass_sn", "numpart", "numparticlecount"))      # with other (dead) contents
        live = a["itra1"] == int(sc["itime"]) + i * int(sc["lsynctime"])
        for k in ARRAYS:
            assert a[k][..., live].tobytes() == b[k][..., live].tobytes(), k
    free = np.concatenate([s["ytra1"][[q["space"] for q in out[i][1]["released"] if q["side"] == "we"]] for i, s in enumerate(runs[0])])
    assert np.unique(free).size > free.size // 2                                # not one value for all


@pytest.mark.gpu
def test_a_step_initialises_exactly_the_new_particles(built):
    from flexpart_amd.engine import RNG_PHILOX
    sc = syn.domainfill_case("fill1")
    sc["itramem"] = np.full(int(sc["npart"]), -7, np.int32)             # nobody is new before the call
    eng = make_engine(sc, 8, rng=RNG_PHILOX)
    d = None
    itime = 0
    for itime in (0, 900):
        st = eng.boundcond_domainfill(itime)
        if itime == 0:
            d = device_state(eng, sc)
            d["itramem"] = np.full(int(sc["npart"]), -7, np.int32)
            move_on(eng, sc, d, 0)
    assert st["n_released"] > 0
    stats = eng.step(900)
    assert stats["n_initialized"] == st["n_released"], (stats, st)
    eng.close()


@pytest.mark.gpu
def test_states_and_refusals(built, tmp_path):
    from flexpart_amd import _lib
    from flexpart_amd.engine import Engine
    sc = syn.domainfill_case("fill1")
    eng = make_engine(sc, 8, init=False)
    lib = eng.lib
    n = C.c_int64(eng.n); npc = C.c_int32(0)
    assert lib.fpx_boundcond_domainfill(eng.h, 0, C.byref(n), C.byref(npc), None) == -3 and b"fpx_domainfill_init first" in lib.fpx_last_error()
    assert lib.fpx_boundcond_output(eng.h, b"x") == -3 and lib.fpx_get_domainfill_acc(eng.h, None, None) == -3
    path = str(tmp_path / "ck.bin")
    eng.checkpoint_write(path, 0, 0)                                   # a handle without the feature: as before
    two = dict(sc); two["numcolumn_we"] = np.array(sc["numcolumn_we"]); two["numcolumn_we"][3, 0] = 2
    with pytest.raises(Exception, match="exactly two release heights"):
        eng.domainfill_init(two)
    high = dict(sc); high["zcolumn_sn"] = np.array(sc["zcolumn_sn"]); high["zcolumn_sn"][5, 4, 0] = 30000.0            # the top of a column of six
    with pytest.raises(Exception, match=r"reaches height\(nz\)"):
        eng.domainfill_init(high)
    wide = dict(sc); wide["nx_we"] = np.array([2, 11], np.int32)
    with pytest.raises(Exception, match="nx_we must lie"):
        eng.domainfill_init(wide)
    eng.domainfill_init(sc)
    assert lib.fpx_checkpoint_write(eng.h, path.encode(), 0, 0) == -5 and b"acc_mass" in lib.fpx_last_error()
    eng.close()
    off = dict(sc); off["mdomainfill"] = 0
    eng = make_engine(off, 8, init=False)
    with pytest.raises(Exception, match="mdomainfill = 0"):
        eng.domainfill_init(off)
    eng.close()
    eng = make_engine(sc, 8, init=False)                               # a two-rank host communicator
    cb = _lib.ALLREDUCE_FN(lambda user, send, recv, count, dtype: 0)
    assert lib.fpx_comm_init_host(eng.h, 2, 0, cb, None) == 0
    with pytest.raises(Exception, match="several ranks"):
        eng.domainfill_init(sc)
    eng.close()
    bare = {k: v for k, v in sc.items() if k not in ("pv",)}
    eng = Engine(sc, compute_real_bytes=8, host_real_bytes=8, max_particles=int(sc["npart"]))       # no pv on the device
    eng.domainfill_init(sc)
    n = C.c_int64(eng.n); npc = C.c_int32(0)
    assert lib.fpx_boundcond_domainfill(eng.h, 0, C.byref(n), C.byref(npc), None) == -3 and b"pv of both slots" in lib.fpx_last_error()
    eng.close()
    del bare


@pytest.mark.gpu
def test_warm_start_through_set_acc(built):
    """fpx_set_domainfill_acc: a handle that receives the masses of another one continues as that one does."""
    sc = syn.domainfill_case("fill1")
    a = make_engine(sc, 8)
    a.boundcond_domainfill(0)
    da = device_state(a, sc)
    b = make_engine(sc, 8)
    zero = dict(sc); zero["acc_mass_we"] = 0 * sc["acc_mass_we"]; zero["acc_mass_sn"] = 0 * sc["acc_mass_sn"]
    b.domainfill_init(zero)
    b.set_domainfill_acc(da["acc_mass_we"], da["acc_mass_sn"])
    db = device_state(b, sc)
    same_bits(da, db, ("acc_mass_we", "acc_mass_sn"))
    a.close(); b.close()
