"""The run loops of Engine::run_md against the oracle's loop on trajectories that cross what the loops are built from: steps
enqueued behind a device-side freeze word and replayed after a list rebuild, the second half-kick of NVE riding on the next
step's first pass, the scatter form's fold inside the integrator pass, thermo rows kept on the device, the NHC chain and the
Berendsen factor advanced on the device, the BDP factor drawn on the host between two enqueues.

Every case is hot (6000 K Maxwell velocities, 2 fs steps, PbTe nep.txt) so that at least one list rebuild falls INSIDE the run --
asserted on the oracle's own count (the skin rule of nepo_run_nve, helpers.oracle_skin_moved), which the engine's count must
equal -- and is run with thermo records on every step and on every fifth step (record steps, deferred steps and a last step that
is neither).  The reference is helpers.OracleLoop (one Oracle.compute per step, FP32) or Oracle.run_nve; it is computed once per
ensemble and shared by the cases of a tier.

GPU tier: H.rocksalt_orthogonal((7, 8, 7)), 3,136 atoms, non-cubic; every case in the gather form (the size rule's choice here) and
in the scatter form pinned with set_win_lanes(1) + set_force_form(1); describe() is asserted either way.  nvt_lan / nvt_bao in the
scatter form: (a) the deterministic limit T_coup = 1e300 against the oracle's NVE trajectory, (b) with noise, the resident loop
against the stepwise sequence of the same engine, bit for bit.
CPU tier (kernel emulator; gather form only, nep_scatter.h is device-only): H.pbte_supercell((2, 2, 2)), 2,000 atoms, 20 steps.

Tolerances: check_nve_against_oracle's (positions and velocities 1e-6, T and U rtol 1e-6, stress columns rtol 1e-4 / atol 1e-6)
and the header of parity_cases.py for the final forces, energies and virials against the FP32 oracle's final state
(|df| <= 1e-4 |f| + 2e-5 eV/A, |dw| <= 1e-4 |w| + 1e-4 eV, energies rtol 1e-5 / atol 2e-5)."""
import functools

import numpy as np
import pytest

import helpers as H

SCATTER = "lds_scatter_of_own_halves"
SEAM = "fold_in_integrator_pass"
NEP = H.golden("PbTe", "nep.txt")
T0, DT = 6000.0, 2.0 / H.TIME_UNIT
BDP_SEED, LAN_SEED = 20240924, 2024
# `ensemble nvt_ber 6000 5000 20`, `nvt_nhc 6000 5000 50`, `nvt_bdp 6000 5000 50`
THERMOSTAT = {"ber": (6000.0, 5000.0, 20.0), "nhc": (6000.0, 5000.0, 50.0), "bdp": (6000.0, 5000.0, 50.0)}
NSTEPS = {"gpu": 16, "emu": 20}


@functools.lru_cache(maxsize=None)
def _system(tier):
    if tier == "gpu":
        h, typ, x = H.rocksalt_orthogonal((7, 8, 7), rattle=0.02, seed=9)
    else:
        h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.02, seed=31)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    vel = H.maxwell_velocities(mass, T0, seed=5)  # zero net momentum
    return h, typ, x, mass, vel


@functools.lru_cache(maxsize=None)
def _reference(tier, ens, calls):
    """the oracle's trajectory of `calls` consecutive run calls of `ens`: thermo rows of EVERY step, the final state, the list
    rebuilds (initial build included) -- computed once, read-only"""
    import time
    h, typ, x, mass, vel = _system(tier)
    orc = H.Oracle(NEP)
    t0 = time.time()
    if ens == "nve":
        assert len(calls) == 1
        r = orc.run_nve(typ, h, x, vel, mass, DT, calls[0], precision=32)
        ref = dict(rows=r["thermo"], x=r["pos"], v=r["vel"], pe=r["pe"], f=r["force"], w=r["virial"], rebuilds=r["rebuilds"])
    else:
        loop = H.OracleLoop(orc, typ, h, x, vel, mass, DT, bdp_seed=BDP_SEED if ens == "bdp" else None)
        rows = [loop.run(ens, k, *THERMOSTAT[ens], record_every=1)[0] for k in calls]
        assert np.abs(np.array(loop.factors) - 1.0).max() > 1e-5  # the thermostat really acts
        ref = dict(rows=np.concatenate(rows), x=loop.x, v=loop.v, pe=loop.pe, f=loop.f, w=loop.w, rebuilds=loop.rebuilds)
    print("\n[oracle %s %s %s] %.1f s, list rebuilds (initial one included) %d" % (tier, ens, calls, time.time() - t0, ref["rebuilds"]))
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return ref


def _engine(drv, n, form):
    eng = drv.engine(drv.model(NEP), n)
    if form == "scatter":
        eng.set_win_lanes(1)
        eng.set_force_form(1)
    return eng


def _run(eng, ens, args, nsteps, thermo_every, t_coup=None):
    if ens == "nve":
        return eng.run_nve(args[0], args[1], args[2], DT, nsteps, *args[3:], thermo_every=thermo_every)
    t1, t2, tc = THERMOSTAT.get(ens, (6000.0, 5000.0, None))
    fn = getattr(eng, "run_nvt_" + ens)
    return fn(args[0], args[1], args[2], DT, nsteps, t1, t2, tc if t_coup is None else t_coup, *args[3:], thermo_every=thermo_every)


def _case(drv, tier, ens, form, thermo_every, calls=None, ref_ens=None, t_coup=None):
    """`calls` consecutive run calls of `ens` on one engine against the oracle's trajectory of `ref_ens` (default: the same
    ensemble): all eight thermo columns at every record, the final state, the rebuild count, the form that ran"""
    h, typ, x, mass, vel = _system(tier)
    n = len(typ)
    calls = tuple(calls or (NSTEPS[tier],))
    ref_ens = ref_ens or ens
    ref = _reference(tier, ref_ens, (sum(calls),) if ref_ens == "nve" else calls)  # (NVE has no ramp: one run serves any split)
    assert ref["rebuilds"] - 1 >= 1, "no list rebuild inside the oracle's run: raise the step count"

    eng = _engine(drv, n, form)
    if ens == "bdp":
        eng.bdp_seed(BDP_SEED)
    if ens in ("lan", "bao"):
        eng.lan_seed(LAN_SEED)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)  # Run: initial force before the loop
    rows, rows_ref, done = [], [], 0
    for k in calls:
        th = _run(eng, ens, (h, d_t, d_m, d_x, d_v, d_pe, d_f, d_w), k, thermo_every, t_coup)
        assert th.shape == (k // thermo_every, 8)
        rows.append(th)
        rows_ref.append(ref["rows"][[done + thermo_every * (j + 1) - 1 for j in range(k // thermo_every)]])
        done += k
    rows, rows_ref = np.concatenate(rows), np.concatenate(rows_ref)
    desc, st = eng.describe(), eng.stats()
    xs, vs, pe, f, w = (drv.host(a) for a in (d_x, d_v, d_pe, d_f, d_w))

    H3 = np.asarray(h, dtype=np.float64).reshape(-1)[:9].reshape(3, 3)
    frac = np.linalg.solve(H3, (xs - ref["x"]).reshape(3, n))
    frac -= np.rint(frac)
    dev = dict(pos=np.abs(H3 @ frac).max(), vel=np.abs(vs - ref["v"]).max(),
               T=np.abs(rows[:, 0] / rows_ref[:, 0] - 1.0).max(), U=np.abs(rows[:, 1] / rows_ref[:, 1] - 1.0).max(),
               stress=np.abs(rows[:, 2:] - rows_ref[:, 2:]).max(),
               f=(np.abs(f - ref["f"]) - 1e-4 * np.abs(ref["f"])).max(), pe=(np.abs(pe - ref["pe"]) - 1e-5 * np.abs(ref["pe"])).max(),
               w=(np.abs(w - ref["w"]) - 1e-4 * np.abs(ref["w"])).max(), wrap=np.abs(xs - H.oracle_apply_pbc(h, xs)).max())
    print("\n[%s %s %s thermo_every=%d calls=%s] rebuilds engine %d oracle %d (initial one included), discarded steps %d, records %d\n"
          "  max deviation: positions %.2e A, velocities %.2e, T rel %.2e, U rel %.2e, stress columns abs %.2e\n"
          "  final state, excess over the relative part: forces %.2e eV/A, energies %.2e eV, virials %.2e eV; moved by another wrap %.1e A\n  %s"
          % (tier, ens, form, thermo_every, calls, st.num_rebuild, ref["rebuilds"], st.discarded_steps, len(rows), dev["pos"], dev["vel"],
             dev["T"], dev["U"], dev["stress"], dev["f"], dev["pe"], dev["w"], dev["wrap"], desc))

    assert (SCATTER in desc) == (form == "scatter"), desc
    if form == "scatter" and ens == "nve":
        assert SEAM in desc, desc
    assert st.num_rebuild == ref["rebuilds"], (st.num_rebuild, ref["rebuilds"])
    assert np.isfinite(rows).all() and len(rows) >= 1
    np.testing.assert_allclose(rows[:, 0], rows_ref[:, 0], rtol=1e-6)   # temperature
    np.testing.assert_allclose(rows[:, 1], rows_ref[:, 1], rtol=1e-6)   # potential energy
    np.testing.assert_allclose(rows[:, 2:], rows_ref[:, 2:], rtol=1e-4, atol=1e-6)
    # positions leave the loop wrapped: the oracle's wrap moves no atom by a lattice vector.  (Not array_equal: apply_pbc goes
    # through fractional coordinates and back, H (H^-1 x), which rounds anew on every application -- ~1e-14 A here.)
    assert dev["wrap"] < 1e-9, dev
    assert dev["pos"] < 1e-6 and dev["vel"] < 1e-6, dev
    assert dev["f"] <= 2e-5, dev
    np.testing.assert_allclose(pe, ref["pe"], rtol=1e-5, atol=2e-5)
    assert dev["w"] <= 1e-4, dev  # (scatter form: the exact_virials() exit pass)
    return eng


def _resident_equals_stepwise(drv, ens):
    """nvt_lan / nvt_bao with noise (T_coup = 50) in the pinned scatter form: the device-resident loop against the stepwise
    sequence of the per-call entry points (set_stepwise_loops) on an engine pinned the same way -- bit for bit, with at least one
    list rebuild inside the run"""
    h, typ, x, mass, vel = _system("gpu")
    n, nsteps, out = len(typ), NSTEPS["gpu"], []
    for stepwise in (False, True):
        eng = _engine(drv, n, "scatter")
        eng.set_stepwise_loops(stepwise)
        d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
        d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
        eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
        eng.lan_seed(LAN_SEED)
        th = _run(eng, ens, (h, d_t, d_m, d_x, d_v, d_pe, d_f, d_w), nsteps, 5, t_coup=50.0)
        desc = eng.describe()
        assert SCATTER in desc, desc
        out.append((drv.host(d_x), drv.host(d_v), th, eng.stats().num_rebuild))
    dx, dv = np.abs(out[0][0] - out[1][0]).max(), np.abs(out[0][1] - out[1][1]).max()
    print("\n[gpu %s scatter resident / stepwise] rebuilds %d / %d (initial one included), max|dx| %.2e, max|dv| %.2e, "
          "max rel thermo %.2e" % (ens, out[0][3], out[1][3], dx, dv, np.abs(out[0][2] / out[1][2] - 1.0).max()))
    assert out[0][3] - 1 >= 1 and out[0][3] == out[1][3], (out[0][3], out[1][3])
    assert np.array_equal(out[0][1], out[1][1]), dv
    assert np.array_equal(out[0][0], out[1][0]), dx
    np.testing.assert_allclose(out[0][2], out[1][2], rtol=1e-12)
    assert np.abs(out[0][2][:, 0] - _reference("gpu", "nve", (nsteps,))["rows"][[4, 9, 14], 0]).max() > 1.0  # the noise really acts


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


FORMS = ["gather", "scatter"]


@pytest.mark.gpu
@pytest.mark.parametrize("thermo_every", [1, 5])
@pytest.mark.parametrize("form", FORMS)
def test_nve_on_gpu(gpu, form, thermo_every):
    """records on every step; records at steps 5, 10 and 15 of 16: deferred second half-kicks (and deferred folds), and a last
    step that is neither a record nor deferred"""
    _case(gpu, "gpu", "nve", form, thermo_every)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_nve_two_calls_on_gpu(gpu, form):
    """7 + 9 steps on one engine, records every 4 steps of a call (global steps 4, 11, 15), against ONE 16-step oracle run: nothing
    deferred is lost or applied twice across a call boundary"""
    _case(gpu, "gpu", "nve", form, 4, calls=(7, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("thermo_every", [1, 5])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ens", ["ber", "nhc", "bdp"])
def test_thermostat_on_gpu(gpu, ens, form, thermo_every):
    """a frozen and replayed step crosses a thermostat pass: the chain state, the Berendsen factor, the BDP draws and the thermo
    rows must come out as if no step had been enqueued behind the trip; the target ramp (step / nsteps) is part of it"""
    _case(gpu, "gpu", ens, form, thermo_every)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_bdp_two_calls_on_gpu(gpu, form):
    """7 + 9 steps: the generator continues across the calls and no draw is lost to a discarded step (the per-step factors show in
    the temperature rows of every step)"""
    _case(gpu, "gpu", "bdp", form, 1, calls=(7, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("ens", ["lan", "bao"])
def test_langevin_deterministic_limit_in_the_scatter_form_on_gpu(gpu, ens):
    """T_coup = 1e300: c1 = 1, c2 = 0, the thermostat passes change nothing and the loop is velocity Verlet -- the oracle's NVE
    trajectory (zero-momentum initial velocities), with the NVE tolerances"""
    _case(gpu, "gpu", ens, "scatter", 5, ref_ens="nve", t_coup=1e300)


@pytest.mark.gpu
@pytest.mark.parametrize("ens", ["lan", "bao"])
def test_langevin_resident_equals_stepwise_in_the_scatter_form_on_gpu(gpu, ens):
    _resident_equals_stepwise(gpu, ens)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tier: the kernel emulator (gather form)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.parametrize("ens", ["nve", "ber", "nhc", "bdp"])
def test_run_loop_on_emulator(emu, ens):
    _case(emu, "emu", ens, "gather", 5)
