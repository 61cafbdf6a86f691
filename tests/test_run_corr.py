"""Correlators sampled inside the run loops (Engine::run_md with nepmi_corr_attach) against sums formed in numpy from the oracle's
own trajectory: helpers.OracleLoop (and test_run_npt_ber.NptOracle for the barostat) stepped with a trace of the velocities behind
every step -- after the second half-kick and after the thermostat's scaling, as measure.process sees them -- and of the unwrapped
positions, accumulated as new - old around every first half-step like parity_cases.check_unwrapped_positions does.

System and settings are those of test_run_loop_oracle.py: H.rocksalt_orthogonal((7, 8, 7)), 3,136 atoms, 6000 K, 2 fs, 16 steps,
PbTe nep.txt (CPU tier: the emulator's 2,000-atom cell, 20 steps).  Asserted from the oracle's own run: a list rebuild lies strictly
inside the run with a sample of every correlator before it and one at or after it, and the engine's rebuild count is the oracle's.
So samples are taken from two different internal orders, and steps enqueued behind the freeze word are replayed: a sample counted
twice or lost shows in the sums (every origin adds to every lag) and the counters are compared exactly.

Tolerances, propagated from that file's own (each coordinate within 1e-6 A, each velocity component within rtol 1e-6), per lag and
component, on the SUMS S over m = atoms x origins terms:
  MSD: every difference u(t) - u(t - l) is off by at most 2e-6, so by Cauchy-Schwarz |dS| <= 2 sqrt(S m) 2e-6 + m (2e-6)^2;
  VAC: every product is off by at most 2e-6 of itself: |dS| <= 2e-6 sum|v v'|.
The measured deviations are printed as fractions of these bounds."""
import functools

import numpy as np
import pytest

import helpers as H
import test_run_npt_ber as NPT

SCATTER = "lds_scatter_of_own_halves"
NEP = H.golden("PbTe", "nep.txt")
T0, DT = 6000.0, 2.0 / H.TIME_UNIT
NHC = (6000.0, 5000.0, 50.0)  # `ensemble nvt_nhc 6000 5000 50`
NSTEPS = {"gpu": 16, "emu": 20}
MSD, VAC = ("msd", 2, 3), ("vac", 1, 4)  # (quantity, sample interval, correlation steps)
VV_SLOT = 6  # nepmi_stats.launches: the integrator passes


@functools.lru_cache(maxsize=None)
def _system(tier):
    if tier == "gpu":
        h, typ, x = H.rocksalt_orthogonal((7, 8, 7), rattle=0.02, seed=9)
    else:
        h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.02, seed=31)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    vel = H.maxwell_velocities(mass, T0, seed=5)
    return np.array(h, dtype=np.float64).reshape(9), typ, x, mass, vel


class _Trace:
    """mixin of the oracle steppers: u[s], v[s] = unwrapped positions and final velocities behind step s"""

    def _trace_init(self):
        self.u, self.us, self._pre = self.x.copy(), [], []

    def _vv(self, first):
        old = self.x.copy() if first else None
        super()._vv(first)
        if first:
            self.u = self.u + (self.x - old)
            self.us.append(self.u.copy())


class _Loop(_Trace, H.OracleLoop):
    def thermo(self):  # called behind the second half-kick of every step (nvt_nhc: in both thermostat halves), before the scaling
        self._pre.append((self.v.copy(), len(self.factors)))
        return super().thermo()

    def velocities(self, ens):
        if ens == "nve":
            return [v for v, _ in self._pre]
        assert ens == "nhc" and len(self._pre) == 2 * len(self.us)
        return [v * self.factors[k] for v, k in self._pre[1::2]]  # (the factor appended right behind that thermo call)


class _NptLoop(_Trace, NPT.NptOracle):
    pass


@functools.lru_cache(maxsize=None)
def _reference(tier, ens):
    h, typ, x, mass, vel = _system(tier)
    nsteps = NSTEPS[tier]
    orc = H.Oracle(NEP)
    if ens == "npt":
        loop = _NptLoop(orc, typ, h, x, vel, mass, DT)
        loop._trace_init()
        loop.run("iso", nsteps, *NPT._barostat("iso"))
        vs = None
    else:
        loop = _Loop(orc, typ, h, x, vel, mass, DT)
        loop._trace_init()
        loop.run(ens, nsteps, *(NHC if ens == "nhc" else ()), record_every=1)
        vs = np.array(loop.velocities(ens))
    ref = dict(u=np.array(loop.us), v=vs, rebuilds=loop.rebuilds, rebuild_steps=tuple(loop.rebuild_steps), x=loop.x.copy(), vel=loop.v.copy())
    assert len(ref["u"]) == nsteps
    print("\n[oracle %s %s] list rebuilds (initial one included) %d at steps %s" % (tier, ens, ref["rebuilds"], ref["rebuild_steps"]))
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return ref


def _expected(spec, ref, nsteps, n):
    """-> sums, sum|terms| [3, num_corr], origins, samples, 1-based sample steps"""
    quantity, interval, num_corr = spec
    steps = list(range(interval, nsteps + 1, interval))
    frames = (ref["u"] if quantity == "msd" else ref["v"])[[t - 1 for t in steps]].reshape(len(steps), 3, n)
    sums, mags, origins = np.zeros((3, num_corr)), np.zeros((3, num_corr)), 0
    for s in range(num_corr - 1, len(steps)):
        origins += 1
        for lag in range(num_corr):
            t = (frames[s] - frames[s - lag]) ** 2 if quantity == "msd" else frames[s] * frames[s - lag]
            sums[:, lag] += t.sum(axis=1)
            mags[:, lag] += np.abs(t).sum(axis=1)
    return sums, mags, origins, len(steps), steps


def _engine(drv, n, form):
    eng = drv.engine(drv.model(NEP), n)
    if form == "scatter":
        eng.set_win_lanes(1)
        eng.set_force_form(1)
    return eng


def _case(drv, tier, ens, form, specs, calls=None, guard_delay=0, timing=False):
    from gpumd_amd.nep import Correlator
    h, typ, x, mass, vel = _system(tier)
    n, nsteps = len(typ), NSTEPS[tier]
    calls = tuple(calls or (nsteps,))
    assert sum(calls) == nsteps
    ref = _reference(tier, ens)
    inside = [r for r in ref["rebuild_steps"] if 1 < r <= nsteps]
    assert inside, "no list rebuild strictly inside the oracle's run"

    eng = _engine(drv, n, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w, d_u = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n), drv.dev(x.copy())
    eng.set_unwrapped(d_u)
    corrs = [Correlator(eng, *spec) for spec in specs]
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
            eng.run_nve(box, d_t, d_m, DT, k, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
        elif ens == "nhc":
            eng.run_nvt_nhc(box, d_t, d_m, DT, k, *NHC, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
        else:
            p0, pc = NPT._barostat("iso")
            eng.run_npt_ber(box, d_t, d_m, DT, k, NPT.T1, NPT.T2, NPT.TC, p0, pc, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    desc, st = eng.describe(), eng.stats()
    got = [c.read() for c in corrs]
    xs, vs = drv.host(d_x), drv.host(d_v)
    for c in corrs:
        eng.detach(c)
        c.close()

    for spec, (sums, origins, samples) in zip(specs, got):
        exp, mag, exp_origins, exp_samples, steps = _expected(spec, ref, nsteps, n)
        assert any(min(steps) < r <= max(steps) for r in inside), (steps, inside)  # a sample before a rebuild, one at or after it
        assert (samples, origins) == (exp_samples, exp_origins) and origins >= 1, (spec, samples, origins, exp_samples, exp_origins)
        m = n * origins
        if spec[0] == "msd":
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
    return xs, vs, st


def _msd_keeps_the_deferred_kick(drv, tier, form, count_launches):
    """NVE with only an MSD correlator attached: the trajectory is bit-identical to the run without it, and (GPU tier: the launch
    counters of nepmi_engine_stats) the loop makes the same number of integrator passes -- one per deferred step, two per record
    step -- while a VAC correlator that samples every step costs the second pass on every step"""
    plain = _case(drv, tier, "nve", form, (), timing=count_launches)
    msd = _case(drv, tier, "nve", form, (MSD,), timing=count_launches)
    assert np.array_equal(plain[0], msd[0]) and np.array_equal(plain[1], msd[1])
    if count_launches:
        vac = _case(drv, tier, "nve", form, (VAC,), timing=True)
        a, b, c = (int(r[2].launches[VV_SLOT]) for r in (plain, msd, vac))
        print("\n[%s nve %s] integrator passes: nothing attached %d, MSD %d, VAC %d" % (tier, form, a, b, c))
        assert a == b and c > a, (a, b, c)
        assert np.array_equal(plain[0], vac[0]) and np.array_equal(plain[1], vac[1])  # (the half-kicks are rounded separately either way)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


FORMS = ["gather", "scatter"]


@pytest.mark.gpu
@pytest.mark.parametrize("calls", [(16,), (7, 9)])
@pytest.mark.parametrize("form", FORMS)
def test_nve_msd_and_vac_together_on_gpu(gpu, form, calls):
    _case(gpu, "gpu", "nve", form, (MSD, VAC), calls=calls)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_nvt_nhc_vac_sees_the_scaled_velocities_on_gpu(gpu, form):
    _case(gpu, "gpu", "nhc", form, (VAC,))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_npt_ber_msd_on_gpu(gpu, form):
    _case(gpu, "gpu", "npt", form, (MSD,))


@pytest.mark.gpu
def test_guard_band_trip_inside_the_run_samples_once_on_gpu(gpu):
    """scatter form, the guard band narrowed from the 6th force assembly on: that step freezes, the lists are rebuilt and it is
    re-run in the gather form; the samples behind the steps before it stand, its own is taken once"""
    _case(gpu, "gpu", "nve", "scatter", (MSD, VAC), guard_delay=6)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_msd_sample_does_not_end_the_deferred_kick_on_gpu(gpu, form):
    _msd_keeps_the_deferred_kick(gpu, "gpu", form, True)


@pytest.mark.parametrize("calls", [(20,), (7, 13)])
def test_nve_msd_and_vac_together_on_emulator(emu, calls):
    _case(emu, "emu", "nve", "gather", (MSD, VAC), calls=calls)


def test_msd_sample_does_not_end_the_deferred_kick_on_emulator(emu):
    _msd_keeps_the_deferred_kick(emu, "emu", "gather", False)
