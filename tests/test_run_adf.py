"""ADF handles sampled inside the run loops (Engine::run_md and the small-box loop with nepmi_adf_attach) against triplet counts
formed in numpy (test_adf_kernels.expected_counts: all triplets, minimum image, the mask rule and definition D) from the frames of
the oracle's own trajectory at the sample steps.

Systems, oracle frames, temperature, time step and the interval of 2 are those of test_run_rdf.py: a list rebuild lies strictly
inside the run with a sample on either side (asserted from the oracle's run), so the samples come from two internal orders and
steps enqueued behind the freeze word are replayed -- a sample taken twice or lost changes every bin by a whole frame's count.
Two handles: the global form at [0, 4) with 90 bins, and the rows (0,1,1), (1,0,0), (0,0,1) at [2, 5) with 90 bins.

Ambiguous triplets.  The engine's positions agree with the oracle's within 1e-6 A per coordinate (check_nve_against_oracle), so a
leg -- a difference of two positions -- within delta = 2 sqrt(3) 1e-6 A.  A triplet is ambiguous if a leg's distance lies within
delta of a bound, or if its angle lies within (180 / pi) delta (1 / d_ia + 1 / d_ib) of a bin edge; a bin's count may deviate by
the number of such triplets (summed over the samples).  Asserted first: they are at most 1e-3 of the counted ones."""
import functools

import numpy as np
import pytest

import helpers as H
import test_adf_kernels as AK
import test_run_corr as RC
import test_run_npt_ber as NPT
import test_run_rdf as RR

NEP, DT, NSTEPS, SCATTER, VV_SLOT = RC.NEP, RC.DT, RC.NSTEPS, RC.SCATTER, RC.VV_SLOT
BINS, INTERVAL, DELTA, PBC = 90, 2, RR.DELTA, (1, 1, 1)
SPECS = {"global": AK.global_rows(0.0, 4.0),
         "triples": [(0, 1, 1, 2.0, 5.0, 2.0, 5.0), (1, 0, 0, 2.0, 5.0, 2.0, 5.0), (0, 0, 1, 2.0, 5.0, 2.0, 5.0)]}


@functools.lru_cache(maxsize=None)
def _expected(tier, ens, spec):
    """-> counts, ambiguous [M, BINS], 1-based sample steps"""
    h, typ, x, mass, vel = RC._system(tier)
    frames, boxes, _, _, _ = RR._frames(tier, ens)
    steps = list(range(INTERVAL, NSTEPS[tier] + 1, INTERVAL))
    counts = np.zeros((len(SPECS[spec]), BINS), dtype=np.int64)
    amb = np.zeros_like(counts)
    for t in steps:
        c, a = AK.expected_counts(frames[t - 1].reshape(3, -1), typ, boxes[t - 1], PBC, SPECS[spec], BINS, delta=DELTA)
        counts += c
        amb += a
    share = amb.sum() / counts.sum()
    print("\n[expected %s %s %s] %d samples, %d triplets counted, %d ambiguous for delta = %.2e A (share %.1e)"
          % (tier, ens, spec, len(steps), counts.sum(), amb.sum(), DELTA, share))
    assert share <= 1e-3, share
    counts.flags.writeable = False
    amb.flags.writeable = False
    return counts, amb, steps


def _run(drv, tier, ens, form, calls=None, guard_delay=0, adf=("global", "triples"), rdf=False, msd=False, timing=False):
    from gpumd_amd.nep import ADF, RDF, Correlator
    h, typ, x, mass, vel = RC._system(tier)
    n, nsteps = len(typ), NSTEPS[tier]
    calls = tuple(calls or (nsteps,))
    assert sum(calls) == nsteps
    eng = RC._engine(drv, n, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w, d_u = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n), drv.dev(x.copy())
    handles = [ADF(eng, SPECS[s], BINS, INTERVAL, typ, 2) for s in adf]
    if rdf:
        handles.append(RDF(eng, RR.RC_RDF, RR.BINS, INTERVAL, typ, 2))
    if msd:
        eng.set_unwrapped(d_u)
        handles.append(Correlator(eng, *RC.MSD))
    for c in handles:
        eng.attach(c)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)  # Run: initial force before the loop
    if guard_delay:
        assert SCATTER in eng.describe()
        eng.set_option("scatter_guard_delay", guard_delay)
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


def _compare(tag, tier, ens, spec, got):
    counts, ns = got
    exp, amb, steps = _expected(tier, ens, spec)
    rebuild_steps = RR._frames(tier, ens)[2]
    inside = [r for r in rebuild_steps if 1 < r <= NSTEPS[tier]]
    assert inside and any(min(steps) < r <= max(steps) for r in inside), (steps, rebuild_steps)
    assert ns == len(steps), (ns, len(steps))
    dev = np.abs(counts.astype(np.int64) - exp)
    print("\n[%s %s] samples %d, triplets %d (expected %d), bins that differ %d, largest |d count| %d, ambiguous allowed %d"
          % (tag, spec, ns, counts.sum(), exp.sum(), int((dev > 0).sum()), int(dev.max()), int(amb.sum())))
    assert exp.sum() > 0 and (dev <= amb).all(), (int(dev.max()), np.argwhere(dev > amb)[:5])


def _compare_both(tag, tier, ens, out):
    for k, spec in enumerate(("global", "triples")):
        _compare(tag, tier, ens, spec, out["got"][k])


def _nve(drv, tier, form, calls=None):
    out = _run(drv, tier, "nve", form, calls=calls)
    _compare_both("%s nve %s calls=%s" % (tier, form, calls), tier, "nve", out)
    assert (SCATTER in out["desc"]) == (form == "scatter"), out["desc"]
    assert out["st"].num_rebuild == RR._frames(tier, "nve")[3]


def _together(drv, tier, form):
    """ADF + RDF + MSD attached together: each equals its value when attached alone, bit for bit (integer sums; the correlator adds
    its partial sums in a fixed order)"""
    alone_adf = _run(drv, tier, "nve", form)
    alone_rdf = RR._run(drv, tier, "nve", form)
    alone_msd = RR._run(drv, tier, "nve", form, msd=True, rdf=False)
    out = _run(drv, tier, "nve", form, rdf=True, msd=True)
    _compare_both("%s nve %s adf + rdf + msd" % (tier, form), tier, "nve", out)
    for k in (0, 1):
        assert np.array_equal(out["got"][k][0], alone_adf["got"][k][0]) and out["got"][k][1] == alone_adf["got"][k][1]
    for a, b in zip(out["got"][2], alone_rdf["got"][0]):
        assert np.array_equal(a, b)
    for a, b in zip(out["got"][3], alone_msd["got"][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(out["x"], alone_adf["x"]) and np.array_equal(out["x"], alone_msd["x"])


def _keeps_the_deferred_kick(drv, tier, form, count_launches):
    """an ADF sample reads positions only: the trajectory is bit-identical to the run with nothing attached and (GPU tier: the launch
    counters of nepmi_engine_stats) the loop makes the same number of integrator passes"""
    plain = _run(drv, tier, "nve", form, adf=(), timing=count_launches)
    adf = _run(drv, tier, "nve", form, timing=count_launches)
    assert np.array_equal(plain["x"], adf["x"]) and np.array_equal(plain["v"], adf["v"])
    if count_launches:
        a, b = (int(r["st"].launches[VV_SLOT]) for r in (plain, adf))
        print("\n[%s nve %s] integrator passes: nothing attached %d, ADF attached %d" % (tier, form, a, b))
        assert a == b and a > 0, (a, b)


def _small_box(drv):
    """the loop that steps on the caller's arrays: the 250-atom PbTe cell (19 A thick), 600 K, 1 fs, 6 steps, interval 2; oracle:
    helpers.OracleLoop on the branch the oracle picks itself"""
    from gpumd_amd.nep import ADF
    fr = H.read_xyz_frames(H.golden("PbTe", "model.xyz"))[0]
    orc = H.Oracle(NEP)
    typ = H.types_from_species(fr["species"], orc.symbols)
    n, h, dt, nsteps = fr["n"], np.asarray(fr["h"], dtype=np.float64), 1.0 / H.TIME_UNIT, 6
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 600.0, seed=8)
    x = H.oracle_apply_pbc(h, H.soa(fr["pos"]))
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt, compute=lambda xx: orc.compute(typ, h, xx, precision=32, path=-1))
    exp = {s: np.zeros((len(SPECS[s]), BINS), dtype=np.int64) for s in SPECS}
    amb = {s: np.zeros((len(SPECS[s]), BINS), dtype=np.int64) for s in SPECS}
    for s in range(nsteps):
        loop.run("nve", 1)
        if (s + 1) % INTERVAL == 0:
            for spec in SPECS:
                c, a = AK.expected_counts(loop.x.reshape(3, -1), typ, h, PBC, SPECS[spec], BINS, delta=DELTA)
                exp[spec] += c
                amb[spec] += a
    eng = drv.engine(drv.model(NEP), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    handles = {s: ADF(eng, SPECS[s], BINS, INTERVAL, typ, 2) for s in SPECS}
    for a in handles.values():
        eng.attach(a)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    eng.run_nve(h, d_t, d_m, dt, 2, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    eng.run_nve(h, d_t, d_m, dt, 4, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    for spec, a in handles.items():
        counts, ns = a.read()
        a.close()
        assert amb[spec].sum() <= 1e-3 * exp[spec].sum()
        dev = np.abs(counts.astype(np.int64) - exp[spec])
        print("\n[%s small box %s] samples %d triplets %d, largest |d count| %d, ambiguous %d"
              % (drv.name, spec, ns, exp[spec].sum(), dev.max(), amb[spec].sum()))
        assert ns == nsteps // INTERVAL and exp[spec].sum() > 0
        assert (dev <= amb[spec]).all()


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
    _compare_both("gpu npt_ber", "gpu", "npt", out)
    assert out["st"].num_rebuild == RR._frames("gpu", "npt")[3]


@pytest.mark.gpu
def test_guard_band_trip_inside_the_run_samples_once_on_gpu(gpu):
    """scatter form, the guard band narrowed from the 6th force assembly on: that step freezes, the lists are rebuilt and it is
    re-run in the gather form; 16 steps at interval 2 are 8 samples, not 9"""
    out = _run(gpu, "gpu", "nve", "scatter", guard_delay=6)
    assert SCATTER not in out["desc"] and out["st"].discarded_steps >= 1
    assert out["got"][0][1] == 8 and out["got"][1][1] == 8
    _compare_both("gpu nve guard-band trip", "gpu", "nve", out)


@pytest.mark.gpu
def test_small_box_loop_on_gpu(gpu):
    _small_box(gpu)


@pytest.mark.gpu
def test_adf_rdf_and_msd_together_on_gpu(gpu):
    _together(gpu, "gpu", "gather")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_adf_sample_does_not_end_the_deferred_kick_on_gpu(gpu, form):
    _keeps_the_deferred_kick(gpu, "gpu", form, True)


@pytest.mark.parametrize("calls", [(20,), (7, 13)])
def test_nve_on_emulator(emu, calls):
    _nve(emu, "emu", "gather", calls)


def test_small_box_loop_on_emulator(emu):
    _small_box(emu)


def test_adf_rdf_and_msd_together_on_emulator(emu):
    _together(emu, "emu", "gather")


def test_adf_sample_does_not_end_the_deferred_kick_on_emulator(emu):
    _keeps_the_deferred_kick(emu, "emu", "gather", False)
