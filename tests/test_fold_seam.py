"""GPU tier: single-domain NVE run loops in the scatter form with the fold of the window sums inside the integrator pass behind
it (engine option "fold_seam" = 1, the default: nep_scatter.h, FoldSeamBody) against the fold and the integrator pass as two
launches (option = 0).  The seam forms each force by the fold's own expressions and hands it to the integrator in registers, so
every output must be bit-identical: positions, velocities, forces, energies, virials and the thermo rows.

Every case runs the smallest system of its kind on which the run loop takes the scatter form (pinned through "force_form": the size
rule would pick the gather form), and asserts through describe() that option 1 did run the seam up to the last step.  One case
crosses a veto instead: a window sum too large for the seam freezes the step in its scatter kernel, the step's forces are evaluated
again with the separate kernels on the same lists, and the arrays must still be equal, bit for bit."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

SCATTER = "lds_scatter_of_own_halves"
SEAM = "fold_in_integrator_pass"


@pytest.fixture(scope="module")
def drv():
    return H.GpuDriver()


def _run(drv, model, h, typ, x, mass, temp, seam, calls=(50,), thermo_every=10, dt_fs=2.0, veto=False):
    """one engine, len(calls) consecutive run_nve calls; returns the state after every call"""
    n = len(typ)
    vel = H.maxwell_velocities(mass, temp, seed=4)
    eng = drv.engine(model, n)
    eng.set_fold_seam(seam)
    eng.set_win_lanes(1)
    eng.set_force_form(1)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    r0 = eng.stats().num_rebuild
    out = []
    for nsteps in calls:
        th = eng.run_nve(h, d_t, d_m, dt_fs / H.TIME_UNIT, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=thermo_every)
        d = eng.describe()
        if veto:  # (the steps behind a veto keep the separate kernels, beyond the length of these runs)
            assert SCATTER in d and SEAM not in d and ("seam_vetoes=" in d) == bool(seam), d
        else:
            assert SCATTER in d and (SEAM in d) == bool(seam) and "seam_vetoes=" not in d, d
        out.append({"x": drv.host(d_x), "vel": drv.host(d_v), "f": drv.host(d_f), "pe": drv.host(d_pe), "w": drv.host(d_w),
                    "th": np.asarray(th, dtype=np.float64).reshape(-1, 8)})
    return out, eng.stats().num_rebuild - r0, eng.stats().discarded_steps


def _same(a, b):
    for key in a:
        diff = np.abs(a[key] - b[key]).max() if a[key].size else 0.0
        print("%-4s equal=%s  max|diff|=%.3e" % (key, np.array_equal(a[key], b[key]), diff))
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


def _both(drv, nep, h, typ, x, mass, temp, min_rebuilds=0, **kw):
    model = drv.model(nep)
    (o0, nb0, nd0), (o1, nb1, nd1) = (_run(drv, model, h, typ, x, mass, temp, s, **kw) for s in (0, 1))
    print("list rebuilds inside the run: %d / %d, steps enqueued behind a frozen one: %d / %d" % (nb0, nb1, nd0, nd1))
    assert nb0 >= min_rebuilds and nb1 == nb0, (nb0, nb1)
    if kw.get("veto"):
        assert nd1 > nd0, (nd0, nd1)  # the vetoed step and what was enqueued behind it ran as no-ops and were replayed
    for a, b in zip(o0, o1):
        assert np.abs(a["f"]).max() > 0.0
        _same(a, b)


def _pbte(reps=(3, 3, 3)):
    h, typ, x = H.pbte_supercell(reps, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    return h, typ, x, mass


def test_pbte_nve_with_list_rebuilds(drv):
    """6,750 atoms of PbTe (two types: the type-pure scatter kernel), 2500 K, 50 steps of 2 fs: list rebuilds fall inside the
    run, so steps freeze on the skin check raised by the seam itself and are replayed behind it"""
    h, typ, x, mass = _pbte()
    _both(drv, H.golden("PbTe", "nep.txt"), h, typ, x, mass, 2500.0, min_rebuilds=1)


@pytest.mark.parametrize("thermo_every,nsteps", [(1, 20), (7, 50), (10, 1), (10, 2)])
def test_record_steps_and_deferred_steps(drv, thermo_every, nsteps):
    """every step a record (the seam stores the force and does the second half-kick only); records every 7 steps (deferred and
    record steps alternate, the last step is neither a multiple of 7 nor deferred); calls of one and of two steps"""
    h, typ, x, mass = _pbte()
    _both(drv, H.golden("PbTe", "nep.txt"), h, typ, x, mass, 2500.0, calls=(nsteps,), thermo_every=thermo_every)


def test_two_calls_on_one_engine(drv):
    """nothing deferred crosses a call: the state after each of two consecutive calls"""
    h, typ, x, mass = _pbte()
    _both(drv, H.golden("PbTe", "nep.txt"), h, typ, x, mass, 2500.0, calls=(23, 27), thermo_every=5)


def test_zbl_model(drv, tmp_path):
    """the fold adds the ZBL pair force of the atom (Bufs::zbl) behind the window sums"""
    import test_model_variants as V
    h, typ, x, mass = _pbte()
    _both(drv, V.make_typewise_zbl(tmp_path), h, typ, x, mass, 1500.0)


def test_many_type_model(drv):
    """UNEP-v1, 16 types, 13,500 atoms: the many-type scatter kernel writes the rows (the PbTe cases: the two-type kernel); with
    its ZBL term.  15 fcc cells per edge, gently rattled, 300 K: the seam runs throughout"""
    h, typ, x = H.fcc_alloy((15, 15, 15), 3.9, 16, rattle=0.01, seed=8)
    mass = 50.0 + 5.0 * typ.astype(np.float64)
    _both(drv, H.golden("UNEP", "nep.txt"), h, typ, x, mass, 300.0, dt_fs=1.0)


def test_across_a_veto(drv):
    """The same alloy in the 12-cell box of the parity cases (6,912 atoms) at 1500 K writes a window sum beyond the seam's bound
    (fold_guard / the most windows an atom lies in): the step freezes in its scatter kernel before any seam has touched it and
    its forces are evaluated again with the separate kernels, WITHOUT a list rebuild -- the same number of rebuilds as with the
    option off, every array equal bit for bit; describe() counts the veto."""
    h, typ, x = H.fcc_alloy((12, 12, 12), 3.9, 16, seed=8)
    mass = 50.0 + 5.0 * typ.astype(np.float64)
    _both(drv, H.golden("UNEP", "nep.txt"), h, typ, x, mass, 1500.0, dt_fs=1.0, veto=True)
