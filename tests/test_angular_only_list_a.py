"""GPU tier: engine option "angular_only_list_a" = 1 (the default) against 0.

With the option on, the list rebuild of a two-type shape writes the members of list A into the two type-pure streams of the
static window layout as well (PackCodesBody: each at the front of the stream of its type, in list order, list B's members
behind them), and the radial pass (nep_window.h: RadialWin2Body<S, SYNC, LEAN, 1>) walks list A for the angular membership
alone.  Each half of the packed radial sums takes the same members in the same order as before, so q, Fp, energies, the
fixed-point forces and with them positions and velocities must be equal under numpy.array_equal.  The per-step compact list
of the scatter form leaves its wave-synchronous words in another order, and the scatter kernel sums its float virial in walk
order: virials and the pressure columns of the thermo rows may move in their last bits.  Their tolerance is measured, not
chosen: twice the largest difference between option 0's scatter form and the gather form (set_force_form(0)) on the same
positions -- the rounding room two legitimate orders of the same sum already have.

Measured on an MI355X (profiles/r13_list_a_ab.txt has every case): the virial arrays a call or a run returns did not move at all
(they come from the pass over the slot-major compact list, whose type-pure segments keep their order); the pressure columns of
the thermo rows moved by 2e-11 .. 1.3e-10 on entries of 3e-3 .. 5e-2, where option 0's scatter and gather forms differ by
1.8e-10 .. 9.2e-10.

One-type, many-type and run-time shapes keep the classic layout under both values (describe(): list_a=classic), and so does an
engine whose per-step radial list takes the mask form (option "radial_mask": it walks list B's rows by their position)."""
import os

import numpy as np
import pytest

import helpers as H
import parity_cases as P

SYNC = "radial_list=wave_synchronous_words"
SCATTER = "lds_scatter_of_own_halves"
AONLY, CLASSIC = " list_a=angular_only ", " list_a=classic "
EXACT_CALL = ("pe", "f", "q", "fp")
EXACT_RUN = ("x", "vel", "f", "pe")


@pytest.fixture(scope="module")
def drv():
    return H.GpuDriver()


def _engine(drv, model, n, aonly, form=1):
    eng = drv.engine(model, n)
    eng.set_angular_only_list_a(aonly)
    eng.set_win_lanes(1)  # (systems below the size the run loops' rule asks for: the one-lane kernels)
    eng.set_force_form(form)
    return eng


def _per_call(drv, model, h, typ, x, aonly, token, form=1):
    n = len(typ)
    eng = _engine(drv, model, n, aonly, form)
    _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    d = eng.describe()
    assert (SCATTER in d) == (form == 1) and token in d, d
    q = drv.zeros(model.info.dim * n, dtype=np.float32)
    fp = drv.zeros(model.info.dim * n, dtype=np.float32)
    eng.descriptors(q, fp)
    return {"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)}


def _run(drv, model, h, typ, x, mass, temp, aonly, token, nsteps=20, dt_fs=2.0, jit=False, form=1):
    """20 steps with thermo_every=5: steps that record (the OUT instantiation of the scatter kernel) among forces-only ones"""
    n = len(typ)
    vel = H.maxwell_velocities(mass, temp, seed=4)
    eng = _engine(drv, model, n, aonly, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    r0 = eng.stats().num_rebuild
    th = eng.run_nve(h, d_t, d_m, dt_fs / H.TIME_UNIT, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    d = eng.describe()
    print(d)
    assert (SYNC in d and SCATTER in d) == (form == 1) and token in d, d
    assert ("shape=jit(" in d) == jit, d
    return {"x": drv.host(d_x), "vel": drv.host(d_v), "f": drv.host(d_f), "pe": drv.host(d_pe), "w": drv.host(d_w),
            "th": np.asarray(th)}, eng.stats().num_rebuild - r0


def _exact(a, b, keys):
    for key in keys:
        print("%-4s equal=%s  max|diff|=%.3e" % (key, np.array_equal(a[key], b[key]), np.abs(a[key] - b[key]).max()))
    for key in keys:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (key, np.abs(a[key] - b[key]).max())


def _totals(w, n):
    return w.reshape(9, n).sum(axis=1)


def _compare_calls(drv, model, h, typ, x, tokens=(CLASSIC, AONLY)):
    """one evaluation in the scatter form under both values, and option 0's gather form as the virial's yardstick"""
    a, b = (_per_call(drv, model, h, typ, x, on, tok) for on, tok in zip((0, 1), tokens))
    g = _per_call(drv, model, h, typ, x, 0, CLASSIC, form=0)
    assert np.abs(a["f"]).max() > 0.0 and np.abs(a["fp"]).max() > 0.0
    _exact(a, b, EXACT_CALL)
    room = np.abs(a["v"] - g["v"]).max()
    moved = np.abs(a["v"] - b["v"]).max()
    print("per call: virial  |scatter(0) - gather(0)| = %.3e   |scatter(1) - scatter(0)| = %.3e" % (room, moved))
    assert moved <= 2.0 * room, (moved, room)
    return a, b


def _compare_runs(drv, model, h, typ, x, mass, temp, tokens=(CLASSIC, AONLY), need_rebuild=True, **kw):
    """20 NVE steps under both values.  The yardstick of the returned virial is option 0's gather form at the final positions;
    the yardstick of the pressure columns of the thermo rows, which the scatter kernel's float sums feed on the way, is the
    same run of option 0 in the gather form (its float forces let the trajectory drift from the fixed-point one by rounding
    over at most 20 steps, which is part of what the two forms legitimately differ by)."""
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, temp, on, tok, **kw) for on, tok in zip((0, 1), tokens))
    print("list rebuilds inside the run: %d / %d" % (nb0, nb1))
    assert nb1 == nb0 and (nb0 >= 1 or not need_rebuild), (nb0, nb1)
    _exact(r0, r1, EXACT_RUN)
    n = len(typ)
    eng = _engine(drv, model, n, 0, form=0)
    _, _, _, wg = H.engine_force(drv, eng, h, typ, r0["x"])
    room_tot = np.abs(_totals(r0["w"], n) - _totals(wg, n)).max()
    moved_tot = np.abs(_totals(r0["w"], n) - _totals(r1["w"], n)).max()
    room_atom = np.abs(r0["w"] - wg).max()
    moved_atom = np.abs(r0["w"] - r1["w"]).max()
    rg, _ = _run(drv, model, h, typ, x, mass, temp, 0, tokens[0], form=0, **kw)
    room_p = np.abs(r0["th"][:, 2:] - rg["th"][:, 2:]).max()
    moved_p = np.abs(r0["th"][:, 2:] - r1["th"][:, 2:]).max()
    print("run: virial totals |scatter(0) - gather(0)| = %.3e  |scatter(1) - scatter(0)| = %.3e   per atom %.3e / %.3e   "
          "thermo pressure columns |scatter(0) - gather(0)| = %.3e  |scatter(1) - scatter(0)| = %.3e  (largest entry %.3e)"
          % (room_tot, moved_tot, room_atom, moved_atom, room_p, moved_p, np.abs(r0["th"][:, 2:]).max()))
    assert np.array_equal(r0["th"][:, :2], r1["th"][:, :2])  # temperature and potential energy
    assert moved_tot <= 2.0 * room_tot, (moved_tot, room_tot)
    assert moved_atom <= 2.0 * room_atom, (moved_atom, room_atom)
    assert moved_p <= 2.0 * room_p, (moved_p, room_p)
    return r0, r1


def _pbte(reps=(3, 3, 3)):
    h, typ, x = H.pbte_supercell(reps, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    return h, typ, x, mass


@pytest.mark.gpu
def test_pbte_nve_with_a_list_rebuild(drv):
    """Case 1.  6,750 atoms of PbTe at 2500 K: one evaluation with the exports, and 20 steps of 2 fs with a list rebuild inside.
    Measured (MI355X): per call, virial |scatter(0) - gather(0)| = 0 and |scatter(1) - scatter(0)| = 0; run, returned virial
    |scatter(0) - gather(0)| = 3.8e-6 per atom, 7.1e-5 on the totals, |scatter(1) - scatter(0)| = 0; pressure columns of the
    thermo rows |scatter(0) - gather(0)| = 6.433e-10, |scatter(1) - scatter(0)| = 1.142e-10 (largest entry 4.0e-2)."""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    _compare_calls(drv, model, h, typ, x)
    _compare_runs(drv, model, h, typ, x, mass, 2500.0)


@pytest.mark.gpu
def test_pbte_with_typewise_zbl(drv, tmp_path):
    """Case 2a"""
    import test_model_variants as V
    h, typ, x, mass = _pbte()
    model = drv.model(V.make_typewise_zbl(tmp_path))
    _compare_calls(drv, model, h, typ, x)
    _compare_runs(drv, model, h, typ, x, mass, 2500.0)


@pytest.mark.gpu
@pytest.mark.parametrize("cutoff", ["7 4 73 8", "6.5 4 73 8", "8 4 7.2 3.6 73 8", "4.2 4.19 73 24"],
                         ids=["rc7", "rc6.5", "per_type", "angular_within_the_band_of_radial"])
def test_pbte_with_other_cutoffs(drv, tmp_path, cutoff):
    """Case 2b-d.  The last one puts the angular cutoff 0.01 A below the radial one: a member of list A is then inside, outside
    or in the band of either cutoff independently -- no walk may take `inside the angular cutoff` for `inside the radial one`
    or the other way round, and the two near-band tests (list A's against the angular cutoff, the streams' against the radial
    one) each retake their own decision."""
    import test_model_variants as V
    L = V._pbte_lines()
    assert L[1].startswith("cutoff")
    model = drv.model(V._write(tmp_path, "cut.txt", [L[0], "cutoff " + cutoff] + L[2:]))
    h, typ, x, mass = _pbte()
    _compare_calls(drv, model, h, typ, x)
    _compare_runs(drv, model, h, typ, x, mass, 1500.0, need_rebuild=False)


@pytest.mark.gpu
def test_pbte_b_shape(drv):
    """Case 3a.  The second compiled two-type shape"""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep_B.txt"))
    a, _ = _compare_calls(drv, model, h, typ, x)
    _compare_runs(drv, model, h, typ, x, mass, 1500.0, need_rebuild=False)


@pytest.mark.gpu
def test_two_type_cover_shape(monkeypatch):
    """Case 3b.  PbTe zero-padded into the compiled two-type cover shape (as tests/test_gpu_parity.py forces it)"""
    monkeypatch.setenv("NEPMI_JIT", "2")
    monkeypatch.setenv("NEPMI_FORCE_COVER", "1")
    drv = H.GpuDriver()
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    eng = _engine(drv, model, len(typ), 1)
    H.engine_force(drv, eng, h, typ, x)
    assert "shape=cover(" in eng.describe() and AONLY in eng.describe(), eng.describe()
    _compare_calls(drv, model, h, typ, x)
    _compare_runs(drv, model, h, typ, x, mass, 1500.0, need_rebuild=False)


def _resolves_to_classic(drv, model, h, typ, x):
    out = []
    for on in (0, 1):
        eng = _engine(drv, model, len(typ), on)
        _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        d = eng.describe()
        print(d)
        assert CLASSIC in d and AONLY not in d, d
        out.append({"pe": pe, "f": f, "v": v})
    assert np.abs(out[0]["f"]).max() > 0.0
    _exact(out[0], out[1], ("pe", "f", "v"))
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C-2022", "BaZrO3"])
def test_one_type_and_three_types_keep_the_classic_layout(drv, name):
    """Case 4a, 4b"""
    nep_rel, build, _ = P.MODELS[name]
    h, typ, x = build()
    _resolves_to_classic(drv, drv.model(H.golden(*nep_rel.split("/"))), h, typ, x)


@pytest.mark.gpu
def test_carbon_2024_on_its_jit_core_keeps_the_classic_layout(monkeypatch):
    """Case 4c.  One type on a prebuilt JIT core (NEPMI_JIT=2: a prebuilt core or none, never the compiler)"""
    monkeypatch.setenv("NEPMI_JIT", "2")
    drv = H.GpuDriver()
    nep_rel, build, _ = P.MODELS["C-2024-window"]
    h, typ, x = build()
    d = _resolves_to_classic(drv, drv.model(H.golden(*nep_rel.split("/"))), h, typ, x)
    assert "shape=jit(" in d, d


@pytest.mark.gpu
def test_mask_form_keeps_the_classic_layout(drv):
    """the mask form of the per-step radial list reads list B's rows by their position: with "radial_mask" the option resolves
    to 0, and switching the mask form off again brings the layout back at the rebuild the switch asks for"""
    h, typ, x, _ = _pbte((2, 2, 2))
    model = drv.model(H.golden("PbTe", "nep.txt"))
    eng = _engine(drv, model, len(typ), 1)
    eng.set_option("radial_mask", 1)
    _, pe0, f0, _ = H.engine_force(drv, eng, h, typ, x)
    assert CLASSIC in eng.describe(), eng.describe()
    eng.set_option("radial_mask", 0)
    _, pe1, f1, _ = H.engine_force(drv, eng, h, typ, x)
    assert AONLY in eng.describe(), eng.describe()
    assert np.array_equal(pe0, pe1) and np.array_equal(f0, f1)


def _radial_counts(h, x, rc):
    """neighbours within rc of every atom, minimum image (the cells below are wider than 2 rc)"""
    hm = np.asarray(h, dtype=np.float64).reshape(3, 3)
    r = np.asarray(x, dtype=np.float64).reshape(3, -1).T
    s = r @ np.linalg.inv(hm).T
    counts = np.zeros(len(r), dtype=np.int64)
    for i0 in range(0, len(r), 250):
        ds = s[i0:i0 + 250, None, :] - s[None, :, :]
        ds -= np.round(ds)
        d2 = ((ds @ hm.T) ** 2).sum(axis=2)
        counts[i0:i0 + 250] = (d2 < rc * rc).sum(axis=1) - 1
    return counts


@pytest.mark.gpu
def test_dense_cell_at_the_capacity_of_the_radial_list(drv, tmp_path):
    """Case 5.  2,000 atoms of PbTe compressed until the busiest atom holds exactly as many radial neighbours as the model's
    capacity allows (MN_radial), and a little further until it holds more: the cells are chosen on the CPU from the neighbour
    counts.  At the capacity both values of the option must evaluate, with equal energies and forces, per call and in a run
    on the wave-synchronous words; beyond it both must report the capacity error from the same call."""
    from gpumd_amd import NepmiError
    import test_model_variants as V
    # (MN_radial 62 instead of 73 in the cutoff line: the rattled cell's busiest atom holds 74 neighbours, and the capacity of 78
    # is reached by two per cent of compression, well before the second shell enters the angular cutoff and the angular
    # capacity speaks first)
    L = V._pbte_lines()
    model = drv.model(V._write(tmp_path, "mn62.txt", [L[0], "cutoff 8 4 62 8"] + L[2:]))
    cap, rc = int(model.info.MN_radial), 8.0
    assert cap == 78, cap  # (the reference enlarges MN by 1.25)
    h0, typ, x0 = H.pbte_supercell((2, 2, 2), rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    n = len(typ)
    assert n <= 2000
    skin = 1.0
    cap_verlet = int(cap * (rc + skin) ** 3 / rc ** 3)  # (the engine's Verlet rows: the capacity scaled to the sphere with the skin)
    scales = 1.0 - 0.0025 * np.arange(1, 80)
    fits = []
    for s in scales:
        hs, xs = np.asarray(h0) * s, np.asarray(x0) * s
        fits.append(_radial_counts(hs, xs, rc).max() <= cap and _radial_counts(hs, xs, rc + skin).max() <= cap_verlet)
        if not fits[-1]:
            break
    assert fits[0] and not fits[-1], fits  # (the last cell that fits sits at the capacity or one step of 0.25 % below it)
    picks = [("fits", scales[len(fits) - 2]), ("beyond", scales[len(fits) - 1])]
    for label, s in picks:
        h, x = np.asarray(h0) * s, np.asarray(x0) * s
        said = []
        for on, tok in ((0, CLASSIC), (1, AONLY)):
            eng = _engine(drv, model, n, on)
            d_t, d_m, d_x = drv.dev(typ), drv.dev(mass), drv.dev(x)
            d_v = drv.dev(H.maxwell_velocities(mass, 300.0, seed=4))
            d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
            where, res = "none", None
            try:
                where = "force_compute"
                eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
                f_call = drv.host(d_f)
                where = "run_nve"
                eng.run_nve(h, d_t, d_m, 1.0 / H.TIME_UNIT, 5, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
                assert tok in eng.describe(), eng.describe()
                where, res = "none", {"f_call": f_call, "f": drv.host(d_f), "pe": drv.host(d_pe), "x": drv.host(d_x)}
            except NepmiError as e:
                assert "capacity" in str(e), e
            said.append((where, res))
        print(label, "scale %.4f busiest atom %d of %d:" % (s, _radial_counts(h, x, rc).max(), cap), [w for w, _ in said])
        assert said[0][0] == said[1][0], said
        if label == "beyond":
            assert said[0][0] != "none", "the cell beyond the capacity must be refused"
        else:
            assert said[0][0] == "none", "the cell that fits must evaluate"
        if said[0][1] is not None:
            _exact(said[0][1], said[1][1], ("f_call", "f", "pe", "x"))


@pytest.mark.gpu
@pytest.mark.parametrize("ghosts", [0, 1], ids=["forward_ghosts", "reverse_ghosts"])
def test_decomposed_run_on_two_ranks(monkeypatch, ghosts):
    """Case 6.  Two ranks as threads over the in-process device transport (32,000 atoms), the scatter form pinned.  The local
    engines are not reachable from here: the option's default comes from the environment, and each rank's describe() names it."""
    import test_dist as T
    import test_dist_inproc as TI
    if not os.path.exists(TI.LIB["gpu"]):
        pytest.skip("tests/inproc transports not built")
    from gpumd_amd.dist import DistMD
    spec = dict(T._spec("gpu", "PbTe-reps", (8, 4, 4), (2, 1, 1), "nve", 20, 3000.0, ghosts=ghosts), force_form=1, thermo_every=5)
    said = []
    close = DistMD.close

    def close_and_tell(self):
        if getattr(self, "handle", None):
            said.append(self.engine_describe())
        close(self)

    monkeypatch.setattr(DistMD, "close", close_and_tell)
    out = []
    for on, token in (("0", CLASSIC), ("1", AONLY)):
        monkeypatch.setenv("NEPMI_ANGULAR_ONLY_LIST_A", on)
        del said[:]
        out.append(TI._run_threads(2, spec))
        print(said)
        assert len(said) == 2 and all(SYNC in d and SCATTER in d and token in d for d in said), said
    # the yardstick of the virial and the pressure columns: option 0 in the gather form (the same recipe as _compare_runs; the
    # gather form's float forces let the trajectory drift from the scatter form's, which only widens the room a little)
    monkeypatch.setenv("NEPMI_ANGULAR_ONLY_LIST_A", "0")
    gather = TI._run_threads(2, dict(spec, force_form=0))
    for ra, rb, rg in zip(out[0], out[1], gather):
        assert int(ra["ndec"]) == int(rb["ndec"]) and int(ra["reverse"]) == ghosts and int(rb["reverse"]) == ghosts
        assert int(ra["nhand"]) == 0 and int(rb["nhand"]) == 0  # (no hand-over to the gather form)
        for key in ("i0", "f0", "i1", "x1", "v1", "f1"):
            assert np.array_equal(ra[key], rb[key]), (key, np.abs(ra[key] - rb[key]).max())
        # temperature and potential energy of the thermo rows; the pressure columns and the virial follow the walk order
        assert np.array_equal(np.asarray(ra["th"])[:, :2], np.asarray(rb["th"])[:, :2])
        assert np.array_equal(np.asarray(ra["th1"])[:2], np.asarray(rb["th1"])[:2])
        for key in ("th", "th1", "w1"):
            room, moved = np.abs(ra[key] - rg[key]).max(), np.abs(ra[key] - rb[key]).max()
            print("%-3s |scatter(0) - gather(0)| = %.3e   |scatter(1) - scatter(0)| = %.3e" % (key, room, moved))
            assert moved <= 2.0 * room, (key, moved, room)


def test_emulator_twin_knows_the_layout():
    """Case 7, emulator tier: the emulator's radial pass is the same template on the same list words, so it is taught the
    layout -- both states run, describe() names them, and every returned array is equal (the emulator has no scatter kernel:
    its compact list is the slot-major one, whose type-pure segments keep their order, virials included)"""
    drv = H.EmuDriver()
    h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.03, seed=17)
    model = drv.model(H.golden("PbTe", "nep.txt"))
    out = []
    for on, tok in ((0, CLASSIC), (1, AONLY)):
        eng = drv.engine(model, len(typ))
        eng.set_angular_only_list_a(on)
        eng.set_win_lanes(1)
        _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        d = eng.describe()
        assert SCATTER not in d and tok in d, d
        q = drv.zeros(model.info.dim * len(typ), dtype=np.float32)
        fp = drv.zeros(model.info.dim * len(typ), dtype=np.float32)
        eng.descriptors(q, fp)
        out.append({"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)})
    assert np.abs(out[0]["f"]).max() > 0.0
    _exact(out[0], out[1], ("pe", "f", "v", "q", "fp"))
