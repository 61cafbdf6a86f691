"""GPU tier: engine option "rebuild_fast_pack" = 1 (the default) against 0.

With the option on, the list rebuild drops work its result does not need: the list builders of a two-type shape hand every
accepted neighbour's type to the packing of the list words as one bit per entry (nep_bodies.h: TypeBitRows, PackCodesTypedBody
-- no PosQ gather per entry), the bricks' statistics and window tables come from one wavefront per brick (TileStatsWaveBody),
and the host looks at the flags once behind the builder.  Every list word, table entry, maximum and flag is the same integer
either way.  The list words feed float sums in list order, so any difference in order or padding shows in the bits of q: every
comparison here is numpy.array_equal, between two engines that differ in the option alone."""
import os

import numpy as np
import pytest

import helpers as H
import parity_cases as P

SYNC = "radial_list=wave_synchronous_words"
MASK = "radial_list=inside_bits_over_the_verlet_words"
SCATTER = "lds_scatter_of_own_halves"
FAST, CLASSIC = " rebuild=fast_pack", " rebuild=classic"
TYPED = " rebuild=fast_pack(types_from_the_builder)"


@pytest.fixture(scope="module")
def drv():
    return H.GpuDriver()


def _engine(drv, model, n, fast, aonly=1, mask=0, pin=True):
    eng = drv.engine(model, n)
    eng.set_rebuild_fast_pack(fast)
    eng.set_angular_only_list_a(aonly)
    if mask:
        eng.set_option("radial_mask", 1)
    if pin:  # (systems below the size the run loops' rule asks for: the one-lane scatter form)
        eng.set_win_lanes(1)
        eng.set_force_form(1)
    return eng


def _per_call(drv, model, h, typ, x, fast, token, scatter=True, **kw):
    n = len(typ)
    eng = _engine(drv, model, n, fast, **kw)
    _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    d = eng.describe()
    print(d)
    assert (SCATTER in d) == scatter and token in d, d
    q = drv.zeros(model.info.dim * n, dtype=np.float32)
    fp = drv.zeros(model.info.dim * n, dtype=np.float32)
    eng.descriptors(q, fp)
    return {"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)}


def _run(drv, model, h, typ, x, mass, temp, fast, token, nsteps=60, dt_fs=2.0, said=(SYNC, SCATTER), **kw):
    """thermo_every=5: steps that record among forces-only ones"""
    n = len(typ)
    vel = H.maxwell_velocities(mass, temp, seed=4)
    eng = _engine(drv, model, n, fast, **kw)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    r0 = eng.stats().num_rebuild
    th = eng.run_nve(h, d_t, d_m, dt_fs / H.TIME_UNIT, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    d = eng.describe()
    print(d)
    assert all(s in d for s in said) and token in d, d
    st = eng.stats()
    return {"x": drv.host(d_x), "vel": drv.host(d_v), "f": drv.host(d_f), "pe": drv.host(d_pe), "w": drv.host(d_w),
            "th": np.asarray(th), "num_rebuild": np.asarray([st.num_rebuild]), "discarded_steps": np.asarray([st.discarded_steps])}, \
        st.num_rebuild - r0


def _same(a, b):
    for key in a:
        print("%-15s equal=%s  max|diff|=%.3e" % (key, np.array_equal(a[key], b[key]), np.abs(a[key] - b[key]).max()))
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (key, np.abs(a[key] - b[key]).max())


def _both_calls(drv, model, h, typ, x, token=FAST, **kw):
    a, b = (_per_call(drv, model, h, typ, x, on, tok, **kw) for on, tok in ((0, CLASSIC), (1, token)))
    assert np.abs(a["f"]).max() > 0.0 and np.abs(a["fp"]).max() > 0.0
    _same(a, b)


def _both_runs(drv, model, h, typ, x, mass, temp, token=FAST, need_rebuild=True, **kw):
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, temp, on, tok, **kw) for on, tok in ((0, CLASSIC), (1, token)))
    print("list rebuilds inside the run: %d / %d" % (nb0, nb1))
    assert nb1 == nb0 and (nb0 >= 1 or not need_rebuild), (nb0, nb1)
    _same(r0, r1)


def _pbte(reps=(3, 3, 3)):
    h, typ, x = H.pbte_supercell(reps, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    return h, typ, x, mass


@pytest.mark.gpu
def test_pbte_call_and_nve_with_a_list_rebuild(drv):
    """6,750 atoms of PbTe (the window kernels): one evaluation with the exports, and 60 steps of 2 fs at 2500 K with at least
    one list rebuild inside the loop"""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    _both_calls(drv, model, h, typ, x, token=TYPED)
    _both_runs(drv, model, h, typ, x, mass, 2500.0, token=TYPED)


@pytest.mark.gpu
def test_pbte_classic_streams(drv):
    """"angular_only_list_a" = 0: the two streams hold list B alone (the type mask starts at list B's first row)"""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    _both_calls(drv, model, h, typ, x, token=TYPED, aonly=0)
    _both_runs(drv, model, h, typ, x, mass, 2500.0, token=TYPED, aonly=0)


@pytest.mark.gpu
def test_pbte_mask_form_of_the_force_assembly(drv):
    """"radial_mask": the scatter form walks list A as the two type-pure runs of words of acode2 / aorig2 / aseg2"""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    _both_calls(drv, model, h, typ, x, token=TYPED, mask=1)
    _both_runs(drv, model, h, typ, x, mass, 2500.0, token=TYPED, mask=1, said=(MASK, SCATTER))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C-2022", "BaZrO3"])
def test_one_type_and_three_types(drv, name):
    """no types are handed over (describe() says so); the tile statistics and the single look change"""
    nep_rel, build, _ = P.MODELS[name]
    h, typ, x = build()
    model = drv.model(H.golden(*nep_rel.split("/")))
    _both_calls(drv, model, h, typ, x, token=FAST + " ")
    if name == "C-2022":
        mass = np.full(len(typ), H.MASS["C"], dtype=np.float64)
        _both_runs(drv, model, h, typ, x, mass, 3000.0, token=FAST + " ", nsteps=40, dt_fs=1.0, need_rebuild=False)


@pytest.mark.gpu
def test_dilute_gas(drv):
    """the dilute gas of tests/test_fused_pair_trip.py (atoms with 0 to 3 neighbours): empty streams, words that are all sentinel"""
    import test_fused_pair_trip as T
    h, typ, x, pos, L = T._sparse_gas()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    _both_calls(drv, model, h, typ, x, token=TYPED)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    _both_runs(drv, model, h, typ, x, mass, 300.0, token=TYPED, nsteps=20, dt_fs=1.0, need_rebuild=False)


@pytest.mark.gpu
def test_dense_cell_at_the_capacity_of_the_radial_list(drv, tmp_path):
    """the cell of tests/test_angular_only_list_a.py compressed until the busiest atom holds exactly the model's capacity of
    radial neighbours (78 of 78): both values evaluate, with equal forces; one step of 0.25 % further (79): both report the
    capacity error, from the same call"""
    from gpumd_amd import NepmiError
    import test_angular_only_list_a as A
    import test_model_variants as V
    L = V._pbte_lines()
    model = drv.model(V._write(tmp_path, "mn62.txt", [L[0], "cutoff 8 4 62 8"] + L[2:]))
    cap, rc, skin = int(model.info.MN_radial), 8.0, 1.0
    assert cap == 78, cap
    h0, typ, x0 = H.pbte_supercell((2, 2, 2), rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    n = len(typ)
    cap_verlet = int(cap * (rc + skin) ** 3 / rc ** 3)
    scales = 1.0 - 0.0025 * np.arange(1, 80)
    fits = []
    for s in scales:
        hs, xs = np.asarray(h0) * s, np.asarray(x0) * s
        fits.append(A._radial_counts(hs, xs, rc).max() <= cap and A._radial_counts(hs, xs, rc + skin).max() <= cap_verlet)
        if not fits[-1]:
            break
    assert fits[0] and not fits[-1], fits
    for label, s in (("fits", scales[len(fits) - 2]), ("beyond", scales[len(fits) - 1])):
        h, x = np.asarray(h0) * s, np.asarray(x0) * s
        said = []
        for on, tok in ((0, CLASSIC), (1, FAST)):
            eng = _engine(drv, model, n, on)
            d_t, d_m, d_x = drv.dev(typ), drv.dev(mass), drv.dev(x)
            d_v = drv.dev(H.maxwell_velocities(mass, 300.0, seed=4))
            d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
            where, res, msg = "none", None, None
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
                msg = str(e)
            said.append((where, res, msg))
        print(label, "scale %.4f busiest atom %d of %d:" % (s, A._radial_counts(h, x, rc).max(), cap), [(w, m) for w, _, m in said])
        assert said[0][0] == said[1][0] and said[0][2] == said[1][2], said  # the same call, the same message
        if label == "beyond":
            assert said[0][0] != "none", "the cell beyond the capacity must be refused"
        else:
            assert said[0][0] == "none", "the cell that fits must evaluate"
            _same(said[0][1], said[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("ghosts", [0, 1], ids=["forward_ghosts", "reverse_ghosts"])
def test_decomposed_run_on_two_ranks(monkeypatch, ghosts):
    """Two ranks as threads over the in-process device transport (32,000 atoms; ghost cells, live bricks, eager reverse slots),
    the scatter form pinned.  The local engines are not reachable from here: the option's default comes from the environment,
    and each rank's describe() names it."""
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
    for on, token in (("0", CLASSIC), ("1", TYPED)):
        monkeypatch.setenv("NEPMI_REBUILD_FAST_PACK", on)
        del said[:]
        out.append(TI._run_threads(2, spec))
        print(said)
        assert len(said) == 2 and all(SYNC in d and SCATTER in d and token in d for d in said), said
    for ra, rb in zip(*out):
        assert int(ra["ndec"]) == int(rb["ndec"]) and int(ra["reverse"]) == ghosts and int(rb["reverse"]) == ghosts
        assert int(ra["nhand"]) == 0 and int(rb["nhand"]) == 0  # (no hand-over to the gather form)
        for key in ("i0", "f0", "i1", "x1", "v1", "f1", "th1", "th", "w1"):
            assert np.array_equal(ra[key], rb[key]), (key, np.abs(ra[key] - rb[key]).max())


@pytest.mark.gpu
def test_box_of_seven_cells_takes_the_fallback_builder(drv):
    """orthogonal rock-salt PbTe, 6 x 6 x 5 cells of 6.57 A: 32.9 A along z are seven cells of 4.5 A, fewer than the eight the
    windows need -- BuildListsBody and the gather kernels run, the fallback builder writes its type bits and nobody reads them"""
    h, typ, x = H.rocksalt_orthogonal((6, 6, 5))
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    model = drv.model(H.golden("PbTe", "nep.txt"))
    out = []
    for on, tok in ((0, CLASSIC), (1, TYPED)):
        out.append(_per_call(drv, model, h, typ, x, on, tok, scatter=False, pin=False))
    assert np.abs(out[0]["f"]).max() > 0.0
    _same(*out)
    _both_runs(drv, model, h, typ, x, mass, 2500.0, token=TYPED, nsteps=40, said=("window=none",), pin=False)


def test_emulator_keeps_the_serial_bodies():
    """emulator tier: no wavefronts and no type rows there -- the option is known, the serial bodies run under both values and
    every returned array is equal"""
    drv = H.EmuDriver()
    h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.03, seed=17)
    model = drv.model(H.golden("PbTe", "nep.txt"))
    out = []
    for on, tok in ((0, CLASSIC), (1, FAST + " ")):
        eng = drv.engine(model, len(typ))
        eng.set_rebuild_fast_pack(on)
        eng.set_win_lanes(1)
        _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        d = eng.describe()
        assert SCATTER not in d and tok in d, d
        q = drv.zeros(model.info.dim * len(typ), dtype=np.float32)
        fp = drv.zeros(model.info.dim * len(typ), dtype=np.float32)
        eng.descriptors(q, fp)
        out.append({"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)})
    assert np.abs(out[0]["f"]).max() > 0.0
    _same(*out)
