"""The mass-weighted velocity autocorrelation (quantity "mvac" of the correlator) sampled inside the run loops, against sums formed
in numpy from the oracle's own trajectory and the masses.  System, settings, oracle trace and engines are those of
test_run_corr.py (3,136 atoms, 6000 K, 2 fs, 16 steps on the GPU; the emulator's 2,000-atom cell, 20 steps); for npt_ber the
velocities behind every step are traced here, after the thermostat's scaling and before the box is rescaled (the barostat moves
positions and box only).

("mvac", interval 1, 4 lags): every step is a sample step, so every step takes its second half-kick as a pass of its own -- as for
VAC -- and a list rebuild strictly inside the run (asserted from the oracle) has samples on both sides.

Bound, as test_run_corr.py derives it for VAC: each velocity component within rtol 1e-6, so each product (w v) v' within 2e-6 of
itself: |dS| <= 2e-6 sum|w v v'| per lag and component.  Counters are compared exactly.  The measured deviations are printed as
fractions of the bound."""
import functools

import numpy as np
import pytest

import helpers as H
import test_run_corr as RC
import test_run_npt_ber as NPT

MVAC = ("mvac", 1, 4)
SCATTER = RC.SCATTER


class _NptLoop(RC._Trace, NPT.NptOracle):
    def _scale(self, kind, p0, pc, th):  # called behind the thermostat's scaling of every step
        self.vs.append(self.v.copy())
        super()._scale(kind, p0, pc, th)


@functools.lru_cache(maxsize=None)
def _reference(tier, ens):
    if ens != "npt":
        return RC._reference(tier, ens)
    h, typ, x, mass, vel = RC._system(tier)
    nsteps = RC.NSTEPS[tier]
    loop = _NptLoop(H.Oracle(RC.NEP), typ, h, x, vel, mass, RC.DT)
    loop._trace_init()
    loop.vs = []
    loop.run("iso", nsteps, *NPT._barostat("iso"))
    ref = dict(v=np.array(loop.vs), rebuilds=loop.rebuilds, rebuild_steps=tuple(loop.rebuild_steps))
    assert len(ref["v"]) == nsteps
    ref["v"].flags.writeable = False
    return ref


def _expected(spec, ref, nsteps, n, mass):
    """-> sums, sum|terms| [3, num_corr], origins, samples, 1-based sample steps"""
    if spec[0] != "mvac":
        return RC._expected(spec, ref, nsteps, n)
    _, interval, num_corr = spec
    steps = list(range(interval, nsteps + 1, interval))
    frames = ref["v"][[t - 1 for t in steps]].reshape(len(steps), 3, n)
    sums, mags, origins = np.zeros((3, num_corr)), np.zeros((3, num_corr)), 0
    for s in range(num_corr - 1, len(steps)):
        origins += 1
        wv = mass[None, :] * frames[s]
        for lag in range(num_corr):
            t = wv * frames[s - lag]
            sums[:, lag] += t.sum(axis=1)
            mags[:, lag] += np.abs(t).sum(axis=1)
    return sums, mags, origins, len(steps), steps


def _case(drv, tier, ens, form, specs, calls=None, guard_delay=0, timing=False, check=True):
    from gpumd_amd.nep import Correlator
    h, typ, x, mass, vel = RC._system(tier)
    n, nsteps = len(typ), RC.NSTEPS[tier]
    calls = tuple(calls or (nsteps,))
    assert sum(calls) == nsteps
    ref = _reference(tier, ens)
    inside = [r for r in ref["rebuild_steps"] if 1 < r <= nsteps]
    assert inside, "no list rebuild strictly inside the oracle's run"

    eng = RC._engine(drv, n, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w, d_u = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n), drv.dev(x.copy())
    eng.set_unwrapped(d_u)
    corrs = [Correlator(eng, *spec, weights=mass if spec[0] == "mvac" else None) for spec in specs]
    for c in corrs:
        eng.attach(c)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)  # Run: initial force before the loop
    if guard_delay:
        assert SCATTER in eng.describe()
        eng.set_option("scatter_guard_delay", guard_delay)  # the narrowed band applies from that force assembly on: inside the run
        eng.set_scatter_guard(0.25)
    if timing:
        eng.set_timing(1)
    box = h.copy()
    for k in calls:
        if ens == "nve":
            eng.run_nve(box, d_t, d_m, RC.DT, k, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
        elif ens == "nhc":
            eng.run_nvt_nhc(box, d_t, d_m, RC.DT, k, *RC.NHC, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
        else:
            p0, pc = NPT._barostat("iso")
            eng.run_npt_ber(box, d_t, d_m, RC.DT, k, NPT.T1, NPT.T2, NPT.TC, p0, pc, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    desc, st = eng.describe(), eng.stats()
    got = [c.read() for c in corrs]
    for c in corrs:
        eng.detach(c)
        c.close()

    for spec, (sums, origins, samples) in zip(specs, got):
        if not check:
            break
        exp, mag, exp_origins, exp_samples, steps = _expected(spec, ref, nsteps, n, mass)
        assert any(min(steps) < r <= max(steps) for r in inside), (steps, inside)  # a sample before a rebuild, one at or after it
        assert (samples, origins) == (exp_samples, exp_origins) and origins >= 1, (spec, samples, origins, exp_samples, exp_origins)
        if spec[0] == "msd":
            m = n * origins
            bound = 2.0 * np.sqrt(exp * m) * 2e-6 + m * (2e-6) ** 2
        else:
            bound = 2e-6 * mag
        dev = np.abs(sums[0] - exp)
        print("\n[%s %s %s calls=%s %s] samples %d origins %d; |dS| per lag (max over components) %s; largest |dS| / bound %.3g"
              % (tier, ens, form, calls, spec, samples, origins, np.array2string(dev.max(axis=0), precision=3),
                 float((dev / bound).max())))
        assert (dev <= bound).all(), (spec, dev, bound)
    print("  rebuilds engine %d oracle %d, discarded steps %d; %s" % (st.num_rebuild, ref["rebuilds"], st.discarded_steps, desc))
    if guard_delay:
        assert SCATTER not in desc, desc  # the hand-over: the gather form has taken over inside the run
        assert st.discarded_steps >= 1    # ... through a frozen and replayed step
    else:
        assert (SCATTER in desc) == (form == "scatter"), desc
        assert st.num_rebuild == ref["rebuilds"], (st.num_rebuild, ref["rebuilds"])
    return got, st


def _together_and_alone(drv, tier, form, alone_specs=None):
    """MVAC, VAC and MSD attached together: each has the bits and counters it has when attached alone (the trajectory does not
    depend on what is attached: test_run_corr.py)"""
    specs = (MVAC, RC.VAC, RC.MSD)
    together, _ = _case(drv, tier, "nve", form, specs)
    for k, spec in enumerate(specs):
        if alone_specs is not None and spec not in alone_specs:
            continue
        (alone,), _ = _case(drv, tier, "nve", form, (spec,), check=False)
        assert alone[0].any() and np.array_equal(alone[0], together[k][0]) and alone[1:] == together[k][1:], spec


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.gpu
@pytest.mark.parametrize("form", RC.FORMS)
def test_nve_on_gpu(gpu, form):
    _case(gpu, "gpu", "nve", form, (MVAC,))


@pytest.mark.gpu
def test_nve_in_two_calls_on_gpu(gpu):
    _case(gpu, "gpu", "nve", "gather", (MVAC,), calls=(7, 9))


@pytest.mark.gpu
def test_nvt_nhc_sees_the_scaled_velocities_on_gpu(gpu):
    _case(gpu, "gpu", "nhc", "gather", (MVAC,))


@pytest.mark.gpu
def test_npt_ber_on_gpu(gpu):
    _case(gpu, "gpu", "npt", "gather", (MVAC,))


@pytest.mark.gpu
def test_guard_band_trip_inside_the_run_samples_once_on_gpu(gpu):
    """scatter form, the guard band narrowed from the 6th force assembly on: that step freezes, the lists are rebuilt and it is
    re-run in the gather form; the samples behind the steps before it stand, its own is taken once"""
    _case(gpu, "gpu", "nve", "scatter", (MVAC,), guard_delay=6)


@pytest.mark.gpu
@pytest.mark.parametrize("form", RC.FORMS)
def test_together_with_vac_and_msd_on_gpu(gpu, form):
    _together_and_alone(gpu, "gpu", form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", RC.FORMS)
def test_as_many_integrator_passes_as_vac_on_gpu(gpu, form):
    """16 NVE steps sampled on every step: the second half-kick is a pass of its own on every step for MVAC as for VAC -- the launch
    counts of the integrator slot are compared between the two runs (and exceed those of a run with nothing attached)"""
    plain = _case(gpu, "gpu", "nve", form, (), timing=True)[1]
    vac = _case(gpu, "gpu", "nve", form, (RC.VAC,), timing=True)[1]
    mvac = _case(gpu, "gpu", "nve", form, (MVAC,), timing=True)[1]
    a, b, c = (int(s.launches[RC.VV_SLOT]) for s in (plain, vac, mvac))
    print("\n[gpu nve %s] integrator passes: nothing attached %d, VAC %d, MVAC %d" % (form, a, b, c))
    assert b == c and c > a, (a, b, c)


def test_nve_on_emulator(emu):
    _case(emu, "emu", "nve", "gather", (MVAC,))


def test_nve_in_two_calls_on_emulator(emu):
    _case(emu, "emu", "nve", "gather", (MVAC,), calls=(7, 13))


def test_together_with_vac_and_msd_on_emulator(emu):
    """(the emulator steps slowly: all three are checked against the oracle together, MVAC alone is run for the comparison of bits)"""
    _together_and_alone(emu, "emu", "gather", alone_specs=(MVAC,))
