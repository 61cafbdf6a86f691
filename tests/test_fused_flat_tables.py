"""GPU tier: the fused angular kernel on its flat-table LDS image (engine option "angular_flat_tables" = 1, the default: a
neuron's bias and output weight as one read, the descriptor scalers read before the invariants, the radial coefficient rows of a
lane's own channels in whole 16-byte groups with a row of zeros where lane 1 has a channel less) against the first image
(option = 0).  The fma chains are the same operands in the same order, so every returned array must be equal under
numpy.array_equal: energies, forces, virials, the exported descriptor and Fp, and the state and thermo rows of run loops.

The one term the flat form adds is Fp x 0 of the zero row on lane 1, which can turn a half sum of exactly -0 into +0 and
nothing else; array_equal does not tell the two zeros apart.

Shapes: PbTe-A has 7 radial channels (lane 1 is one short: the branch the flat table removes) and 7 basis functions (rows padded
from 7 to 8); PbTe-B has 5 and 9 (padded to 12); BaZrO3 has 9 and 9 on three types (a last trip of the table loop with one
block); carbon has 11 channels, 11 basis functions (12: no padding of k), one type, and keeps the one-record loops.  None of
the golden models has an even channel count, so the case without a zero row is not covered here.

The fused kernel exists on the device only; on the emulator the option is accepted and changes nothing
(test_option_is_accepted_where_the_kernel_does_not_exist)."""
import numpy as np
import pytest

import helpers as H
import parity_cases as P

FUSED = "partial_forces_in_one_kernel"
FLAT = "flat_tables"


@pytest.fixture(scope="module")
def drv():
    return H.GpuDriver()


def _per_call(drv, model, h, typ, x, flat):
    n = len(typ)
    eng = drv.engine(model, n)
    eng.set_angular_flat_tables(flat)
    _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    d = eng.describe()
    assert FUSED in d and (FLAT in d) == bool(flat), d
    q = drv.zeros(model.info.dim * n, dtype=np.float32)
    fp = drv.zeros(model.info.dim * n, dtype=np.float32)
    eng.descriptors(q, fp)
    return {"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)}


def _run(drv, model, h, typ, x, mass, temp, flat, nsteps=20, dt_fs=2.0, force_form=1):
    n = len(typ)
    vel = H.maxwell_velocities(mass, temp, seed=4)
    eng = drv.engine(model, n)
    eng.set_angular_flat_tables(flat)
    if force_form is not None:  # (systems below the size the run loops' rule asks for: pin the one-lane scatter form)
        eng.set_win_lanes(1)
        eng.set_force_form(force_form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    r0 = eng.stats().num_rebuild
    th = eng.run_nve(h, d_t, d_m, dt_fs / H.TIME_UNIT, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    d = eng.describe()
    assert FUSED in d and (FLAT in d) == bool(flat), d
    return {"x": drv.host(d_x), "vel": drv.host(d_v), "f": drv.host(d_f), "pe": drv.host(d_pe), "w": drv.host(d_w),
            "th": np.asarray(th)}, eng.stats().num_rebuild - r0


def _same(a, b):
    for key in a:
        print("%-4s equal=%s  max|diff|=%.3e" % (key, np.array_equal(a[key], b[key]), np.abs(a[key] - b[key]).max()))
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (key, np.abs(a[key] - b[key]).max())


def _pbte(reps=(3, 3, 3)):
    h, typ, x = H.pbte_supercell(reps, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    return h, typ, x, mass


@pytest.mark.gpu
def test_pbte_nve_with_a_list_rebuild(drv):
    """6,750 atoms of PbTe at 2500 K, one evaluation with the exports and 20 steps of 2 fs with a list rebuild inside"""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    a, b = (_per_call(drv, model, h, typ, x, flat) for flat in (0, 1))
    assert np.abs(a["f"]).max() > 0.0 and np.abs(a["fp"]).max() > 0.0
    _same(a, b)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 2500.0, flat) for flat in (0, 1))
    print("list rebuilds inside the run: %d / %d" % (nb0, nb1))
    assert nb0 >= 1 and nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
def test_pbte_with_typewise_zbl(drv, tmp_path):
    """ZBL stays per pair inside the record loops; the per-atom phases around them must leave it alone"""
    import test_model_variants as V
    h, typ, x, mass = _pbte()
    model = drv.model(V.make_typewise_zbl(tmp_path))
    _same(*(_per_call(drv, model, h, typ, x, flat) for flat in (0, 1)))
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 1500.0, flat) for flat in (0, 1))
    assert nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["PbTe-B", "BaZrO3", "C-2022", "PbTe-ortho", "water-model"])
def test_other_shapes(drv, name):
    """the models of tests/test_gpu_parity.py's fused-against-separate test: other paddings of the table, three types (an odd
    type count: the table loop's last trip has one block), one type with the one-record loops, and a model served by a cover
    shape"""
    nep_rel, build, _ = P.MODELS[name]
    h, typ, x = build()
    model = drv.model(H.golden(*nep_rel.split("/")))
    a, b = (_per_call(drv, model, h, typ, x, flat) for flat in (0, 1))
    assert np.abs(a["f"]).max() > 0.0
    _same(a, b)


@pytest.mark.gpu
def test_atoms_with_zero_to_three_angular_neighbours(drv):
    """the dilute gas of tests/test_fused_pair_trip.py: atoms whose record loops make no trip at all go through the per-atom
    phases all the same"""
    import test_fused_pair_trip as T
    h, typ, x, pos, L = T._sparse_gas()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    a, b = (_per_call(drv, model, h, typ, x, flat) for flat in (0, 1))
    assert np.abs(a["f"]).max() > 0.0
    _same(a, b)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 300.0, flat, dt_fs=1.0, force_form=None) for flat in (0, 1))
    assert nb0 == nb1
    _same(r0, r1)


@pytest.mark.gpu
def test_decomposed_run_with_forward_ghosts(monkeypatch):
    """Two ranks as threads over the in-process device transport, forward-mode ghosts: the local engines carry ghost levels and
    are not reachable from here, so the option's default comes from the environment."""
    import test_dist as T
    import test_dist_inproc as TI
    import os
    if not os.path.exists(TI.LIB["gpu"]):
        pytest.skip("tests/inproc transports not built")
    spec = T._spec("gpu", "PbTe-reps", (4, 2, 2), (2, 1, 1), "nve", 20, 3000.0, ghosts=0)
    out = []
    for flat in ("0", "1"):
        monkeypatch.setenv("NEPMI_ANGULAR_FLAT_TABLES", flat)
        out.append(TI._run_threads(2, spec))
    for ra, rb in zip(*out):
        assert int(ra["ndec"]) == int(rb["ndec"]) and int(ra["reverse"]) == 0
        for key in ("i0", "f0", "i1", "x1", "v1", "f1", "th1"):
            assert np.array_equal(ra[key], rb[key]), (key, np.abs(ra[key] - rb[key]).max())


def test_option_is_accepted_where_the_kernel_does_not_exist():
    """emulator tier: no fused kernel -- the option is known, describe() names no flat tables, the forces do not move"""
    drv = H.EmuDriver()
    h, typ, x = H.pbte_supercell((2, 2, 2))
    model = drv.model(H.golden("PbTe", "nep.txt"))
    out = []
    for flat in (0, 1):
        eng = drv.engine(model, len(typ))
        eng.set_angular_flat_tables(flat)
        _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        assert FLAT not in eng.describe(), eng.describe()
        out.append({"pe": pe, "f": f, "v": v})
    _same(*out)
