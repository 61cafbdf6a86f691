"""RDF handles sampled inside the run loops (Engine::run_md and the small-box loop with nepmi_rdf_attach) against pair counts formed
in numpy (test_rdf_kernels.expected_counts: all pairs, minimum image, the bin rule of rdf.cu:97-118) from the frames of the oracle's
own trajectory at the sample steps.

System and settings are those of test_run_corr.py: H.rocksalt_orthogonal((7, 8, 7), rattle=0.02, seed=9), 3,136 atoms, 45 A thick,
6000 K, 2 fs, 16 steps (CPU tier: the emulator's 2,000-atom triclinic cell, 20 steps); rc = 8 A, 100 bins, interval 2.  Hot enough
that a list rebuild lies strictly inside the run with a sample before it and one at or after it (asserted from the oracle's run): the
samples come from two internal orders and steps enqueued behind the freeze word are replayed -- a sample taken twice or lost changes
every bin by a whole frame's count.

Ambiguous pairs.  The engine's positions agree with the oracle's within 1e-6 A per coordinate (check_nve_against_oracle), so a
distance -- a difference of two positions -- within delta = 2 sqrt(3) 1e-6 A.  A pair whose oracle distance lies within delta of a
bin edge or of rc may fall on either side; a bin's count may deviate by the number of such pairs (summed over the samples).
Asserted first: they are at most 1e-3 of the counted pairs (expected at dr = 0.08 A: about 1e-4).
npt_ber: vsum against sum_s count_s V_s with the oracle stepper's volumes, relative tolerance the box tolerance of
test_run_npt_ber.py (steps x p_coupling x (1e-4 max|p| + 1e-6)), plus the ambiguous pairs' weight."""
import functools

import numpy as np
import pytest

import helpers as H
import test_rdf_kernels as RK
import test_run_corr as RC
import test_run_npt_ber as NPT

NEP, DT, NSTEPS, SCATTER, VV_SLOT = RC.NEP, RC.DT, RC.NSTEPS, RC.SCATTER, RC.VV_SLOT
RC_RDF, BINS, INTERVAL = 8.0, 100, 2
DELTA = 2.0 * np.sqrt(3.0) * 1e-6
PBC = (1, 1, 1)


class _NptFrames(NPT.NptOracle):
    """the positions and the box every step ends with (after the barostat's scaling: what RDF::process sees)"""

    def _scale(self, kind, p0, pc, th):
        super()._scale(kind, p0, pc, th)
        if not hasattr(self, "frames"):
            self.frames, self.frame_boxes = [], []
        self.frames.append(self.x.copy())
        self.frame_boxes.append(self.h.copy())


@functools.lru_cache(maxsize=None)
def _frames(tier, ens):
    """-> (frames [nsteps][3n], boxes [nsteps][9], rebuild_steps, rebuilds, strain_tol)"""
    h, typ, x, mass, vel = RC._system(tier)
    nsteps = NSTEPS[tier]
    if ens == "nve":
        ref = RC._reference(tier, "nve")  # (the unwrapped positions: an RDF does not see the wrap)
        return ref["u"], np.tile(h, (nsteps, 1)), ref["rebuild_steps"], ref["rebuilds"], 0.0
    p0, pc = NPT._barostat("iso")
    loop = _NptFrames(H.Oracle(NEP), typ, h, x, vel, mass, DT)
    rows, _ = loop.run("iso", nsteps, p0, pc)
    strain_tol = nsteps * pc.max() * (1e-4 * np.abs(rows[:, 2:]).max() + 1e-6)
    return np.array(loop.frames), np.array(loop.frame_boxes), tuple(loop.rebuild_steps), loop.rebuilds, strain_tol


@functools.lru_cache(maxsize=None)
def _expected(tier, ens):
    """-> counts, ambiguous, sum_s count_s V_s, sum_s ambiguous_s V_s [P, BINS], 1-based sample steps"""
    h, typ, x, mass, vel = RC._system(tier)
    frames, boxes, _, _, _ = _frames(tier, ens)
    steps = list(range(INTERVAL, NSTEPS[tier] + 1, INTERVAL))
    counts = np.zeros((3, BINS), dtype=np.int64)
    amb, cv, av = np.zeros_like(counts), np.zeros((3, BINS)), np.zeros((3, BINS))
    for t in steps:
        c, a = RK.expected_counts(frames[t - 1].reshape(3, -1), typ, boxes[t - 1], PBC, RC_RDF, BINS, 2, eps_abs=DELTA)
        V = RK.box_volume(boxes[t - 1])
        counts += c
        amb += a
        cv += c * V
        av += a * V
    share = amb.sum() / counts.sum()
    print("\n[expected %s %s] %d samples, %d pairs counted, %d ambiguous for delta = %.2e A (share %.1e)"
          % (tier, ens, len(steps), counts.sum(), amb.sum(), DELTA, share))
    assert share <= 1e-3, share
    for a in (counts, amb, cv, av):
        a.flags.writeable = False
    return counts, amb, cv, av, steps


def _run(drv, tier, ens, form, calls=None, guard_delay=0, msd=False, timing=False, rdf=True):
    from gpumd_amd.nep import RDF, Correlator
    h, typ, x, mass, vel = RC._system(tier)
    n, nsteps = len(typ), NSTEPS[tier]
    calls = tuple(calls or (nsteps,))
    assert sum(calls) == nsteps
    eng = RC._engine(drv, n, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w, d_u = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n), drv.dev(x.copy())
    handles = []
    if rdf:
        handles.append(RDF(eng, RC_RDF, BINS, INTERVAL, typ, 2))
    if msd:
        eng.set_unwrapped(d_u)
        handles.append(Correlator(eng, *RC.MSD))
    for c in handles:
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
        else:
            p0, pc = NPT._barostat("iso")
            eng.run_npt_ber(box, d_t, d_m, DT, k, NPT.T1, NPT.T2, NPT.TC, p0, pc, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    out = dict(desc=eng.describe(), st=eng.stats(), got=[c.read() for c in handles], x=drv.host(d_x), v=drv.host(d_v))
    for c in handles:
        eng.detach(c)
        c.close()
    return out


def _compare(tag, tier, ens, got):
    counts, vsum, ns = got
    exp, amb, cv, av, steps = _expected(tier, ens)
    _, _, rebuild_steps, _, strain_tol = _frames(tier, ens)
    inside = [r for r in rebuild_steps if 1 < r <= NSTEPS[tier]]
    assert inside and any(min(steps) < r <= max(steps) for r in inside), (steps, rebuild_steps)
    assert ns == len(steps), (ns, len(steps))
    dev = np.abs(counts.astype(np.int64) - exp)
    print("\n[%s] samples %d, pairs %d (expected %d), bins that differ %d, largest |d count| %d, ambiguous allowed %d"
          % (tag, ns, counts.sum(), exp.sum(), int((dev > 0).sum()), int(dev.max()), int(amb.sum())))
    assert (dev <= amb).all(), (int(dev.max()), np.argwhere(dev > amb)[:5])
    vdev = np.abs(vsum - cv)
    assert (vdev <= max(strain_tol, 4 * 2.0 ** -52 * len(steps)) * cv + av).all(), float((vdev / np.maximum(cv, 1e-300)).max())


def _nve(drv, tier, form, calls=None):
    out = _run(drv, tier, "nve", form, calls=calls)
    _compare("%s nve %s calls=%s" % (tier, form, calls), tier, "nve", out["got"][0])
    assert (SCATTER in out["desc"]) == (form == "scatter"), out["desc"]
    assert out["st"].num_rebuild == _frames(tier, "nve")[3]


def _with_msd(drv, tier, form):
    out = _run(drv, tier, "nve", form, msd=True)
    _compare("%s nve %s rdf + msd" % (tier, form), tier, "nve", out["got"][0])
    sums, origins, samples = out["got"][1]
    exp, mag, exp_origins, exp_samples, _ = RC._expected(RC.MSD, RC._reference(tier, "nve"), NSTEPS[tier], len(RC._system(tier)[1]))
    m = len(RC._system(tier)[1]) * origins
    assert (samples, origins) == (exp_samples, exp_origins)
    assert (np.abs(sums[0] - exp) <= 2.0 * np.sqrt(exp * m) * 2e-6 + m * (2e-6) ** 2).all()


def _keeps_the_deferred_kick(drv, tier, form, count_launches):
    """an RDF sample reads positions only: the trajectory is bit-identical to the run with nothing attached and (GPU tier: the launch
    counters of nepmi_engine_stats) the loop makes the same number of integrator passes"""
    plain = _run(drv, tier, "nve", form, rdf=False, timing=count_launches)
    rdf = _run(drv, tier, "nve", form, timing=count_launches)
    assert np.array_equal(plain["x"], rdf["x"]) and np.array_equal(plain["v"], rdf["v"])
    if count_launches:
        a, b = (int(r["st"].launches[VV_SLOT]) for r in (plain, rdf))
        print("\n[%s nve %s] integrator passes: nothing attached %d, RDF attached %d" % (tier, form, a, b))
        assert a == b and a > 0, (a, b)


def _small_box(drv):
    """the loop that steps on the caller's arrays: the 250-atom PbTe cell (19 A thick, below 2.5 (rc + skin) of the potential),
    600 K, 1 fs, 6 steps, rc = 6 A, interval 2; oracle: helpers.OracleLoop on the branch the oracle picks itself"""
    from gpumd_amd.nep import RDF
    fr = H.read_xyz_frames(H.golden("PbTe", "model.xyz"))[0]
    orc = H.Oracle(NEP)
    typ = H.types_from_species(fr["species"], orc.symbols)
    n, h, dt, nsteps, rc = fr["n"], np.asarray(fr["h"], dtype=np.float64), 1.0 / H.TIME_UNIT, 6, 6.0
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 600.0, seed=8)
    x = H.oracle_apply_pbc(h, H.soa(fr["pos"]))
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt, compute=lambda xx: orc.compute(typ, h, xx, precision=32, path=-1))
    exp, amb = np.zeros((3, BINS), dtype=np.int64), np.zeros((3, BINS), dtype=np.int64)
    for s in range(nsteps):
        loop.run("nve", 1)
        if (s + 1) % INTERVAL == 0:
            c, a = RK.expected_counts(loop.x.reshape(3, -1), typ, h, PBC, rc, BINS, 2, eps_abs=DELTA)
            exp += c
            amb += a
    assert amb.sum() <= 1e-3 * exp.sum()
    eng = drv.engine(drv.model(NEP), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    r = RDF(eng, rc, BINS, INTERVAL, typ, 2)
    eng.attach(r)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    eng.run_nve(h, d_t, d_m, dt, 2, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    eng.run_nve(h, d_t, d_m, dt, 4, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    counts, vsum, ns = r.read()
    r.close()
    dev = np.abs(counts.astype(np.int64) - exp)
    print("\n[%s small box] samples %d pairs %d, largest |d count| %d, ambiguous %d" % (drv.name, ns, exp.sum(), dev.max(), amb.sum()))
    assert ns == nsteps // INTERVAL and exp.sum() > 0
    assert (dev <= amb).all()


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
def test_nve_on_gpu(gpu, form, calls):
    _nve(gpu, "gpu", form, calls)


@pytest.mark.gpu
def test_npt_ber_on_gpu(gpu):
    out = _run(gpu, "gpu", "npt", "gather")
    _compare("gpu npt_ber", "gpu", "npt", out["got"][0])
    assert out["st"].num_rebuild == _frames("gpu", "npt")[3]


@pytest.mark.gpu
def test_guard_band_trip_inside_the_run_samples_once_on_gpu(gpu):
    """scatter form, the guard band narrowed from the 6th force assembly on: that step freezes, the lists are rebuilt and it is
    re-run in the gather form; 16 steps at interval 2 are 8 samples, not 9"""
    out = _run(gpu, "gpu", "nve", "scatter", guard_delay=6)
    assert SCATTER not in out["desc"] and out["st"].discarded_steps >= 1
    assert out["got"][0][2] == 8
    _compare("gpu nve guard-band trip", "gpu", "nve", out["got"][0])


@pytest.mark.gpu
def test_small_box_loop_on_gpu(gpu):
    _small_box(gpu)


@pytest.mark.gpu
def test_rdf_and_msd_together_on_gpu(gpu):
    _with_msd(gpu, "gpu", "gather")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_rdf_sample_does_not_end_the_deferred_kick_on_gpu(gpu, form):
    _keeps_the_deferred_kick(gpu, "gpu", form, True)


@pytest.mark.parametrize("calls", [(20,), (7, 13)])
def test_nve_on_emulator(emu, calls):
    _nve(emu, "emu", "gather", calls)


def test_small_box_loop_on_emulator(emu):
    _small_box(emu)


def test_rdf_and_msd_together_on_emulator(emu):
    _with_msd(emu, "emu", "gather")


def test_rdf_sample_does_not_end_the_deferred_kick_on_emulator(emu):
    _keeps_the_deferred_kick(emu, "emu", "gather", False)
