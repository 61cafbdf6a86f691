"""Angular-RDF handles sampled inside the run loops (Engine::run_md and the small-box loop with nepmi_ardf_attach) against pair
counts formed in numpy (all ordered pairs, minimum image, the bin rule of include/nepmi.h) from the frames of the oracle's own
trajectory at the sample steps.

System and settings are those of test_run_rdf.py: 3,136 atoms, 6000 K, 2 fs, 16 steps with a list rebuild strictly inside the run
(CPU tier: the emulator's cell, 20 steps); rc = 8 A, 40 radial x 24 azimuth bins, interval 2, columns total + (0,0) + (0,1).

Ambiguous pairs, as in test_run_rdf.py: positions agree with the oracle's within 1e-6 A per coordinate, a distance within
delta = 2 sqrt(3) 1e-6 A.  A pair within delta of an r edge (or of rc) may fall on either side; so may a pair within
delta / (its in-plane distance) of a theta edge (or of +-pi); a pair with an in-plane distance below 1e-3 A counts as ambiguous in
every azimuth bin.  A bin may deviate by the number of pairs that may lie in it and need not (summed over the samples).  Asserted
first, on the oracle's frames alone: ambiguous pairs are at most 1e-3 of the counted pairs.
npt_ber: vsum against sum_s count_s V_s with the oracle stepper's volumes, tolerance as in test_run_rdf.py."""
import functools

import numpy as np
import pytest

import helpers as H
import test_ardf_kernels as AK
import test_rdf_kernels as RK
import test_run_adf as RA
import test_run_corr as RC
import test_run_npt_ber as NPT
import test_run_rdf as RR

NEP, DT, NSTEPS, SCATTER, VV_SLOT = RC.NEP, RC.DT, RC.NSTEPS, RC.SCATTER, RC.VV_SLOT
RCUT, R, T, INTERVAL = 8.0, 40, 24, 2
PAIRS = ((0, 0), (0, 1))
DELTA = RR.DELTA
PBC = (1, 1, 1)


def expected_counts(pos, typ, h9, pbc, rc, nr, nt, pairs, delta):
    """all ordered pairs -> (counts, ambiguous) [C, nr, nt]: `ambiguous` counts, per bin, the pairs that may lie in it within delta
    and need not"""
    Hm = np.asarray(h9, dtype=np.float64).reshape(3, 3)
    s = np.linalg.solve(Hm, pos)
    n = pos.shape[1]
    lo, up, th_up = AK.edges(rc, nr, nt)
    counts = np.zeros((1 + len(pairs), nr, nt), dtype=np.int64)
    amb = np.zeros_like(counts)

    def rbin(d):  # -1: not counted
        w = np.searchsorted(up, d, side="left")
        return np.where((d > lo[0]) & (d <= rc) & (w < nr), np.minimum(w, nr - 1), -1)

    def tbin(th):
        th = np.where(th > np.pi, th - 2 * np.pi, np.where(th < -np.pi, th + 2 * np.pi, th))
        return np.minimum(np.searchsorted(th_up, th, side="left"), nt - 1)

    for i0 in range(0, n, 256):
        i1 = min(n, i0 + 256)
        ds = s[:, None, :] - s[:, i0:i1, None]
        for d in range(3):
            if pbc[d]:
                ds[d] -= np.round(ds[d])
        dv = np.einsum("ab,bij->aij", Hm, ds)
        d2 = (dv * dv).sum(axis=0)
        ii, jj = np.meshgrid(np.arange(i0, i1), np.arange(n), indexing="ij")
        sel = (jj != ii) & (d2 <= (rc + 2 * delta) ** 2)
        dist, dx, dy, ti, tj = np.sqrt(d2[sel]), dv[0][sel], dv[1][sel], typ[ii[sel]], typ[jj[sel]]
        theta = np.arctan2(dy, dx)
        rxy = np.hypot(dx, dy)
        dth = delta / np.maximum(rxy, 1e-3)
        w, w0, w1 = rbin(dist), rbin(dist - delta), rbin(dist + delta)
        t, t0, t1 = tbin(theta), tbin(theta - dth), tbin(theta + dth)
        member = [np.ones(len(dist), dtype=bool)] + [(ti == a) & (tj == b) for a, b in pairs]
        ok = w >= 0
        for c, m in enumerate(member):
            np.add.at(counts[c], (w[ok & m], t[ok & m]), 1)
        odd = (w0 != w1) | (t0 != t1) | (rxy < 1e-3)
        for k in np.flatnonzero(odd):
            ws = {int(w0[k]), int(w[k]), int(w1[k])} - {-1}
            ts = set(range(nt)) if rxy[k] < 1e-3 else {int(t0[k]), int(t[k]), int(t1[k])}
            for c, m in enumerate(member):
                if m[k]:
                    for a in ws:
                        for b in ts:
                            amb[c, a, b] += 1
    return counts, amb


@functools.lru_cache(maxsize=None)
def _expected(tier, ens):
    """-> counts, ambiguous, sum_s count_s V_s, sum_s ambiguous_s V_s [C, R, T], 1-based sample steps"""
    h, typ, x, mass, vel = RC._system(tier)
    frames, boxes, _, _, _ = RR._frames(tier, ens)
    steps = list(range(INTERVAL, NSTEPS[tier] + 1, INTERVAL))
    counts = np.zeros((1 + len(PAIRS), R, T), dtype=np.int64)
    amb, cv, av = np.zeros_like(counts), np.zeros(counts.shape), np.zeros(counts.shape)
    for t in steps:
        c, a = expected_counts(frames[t - 1].reshape(3, -1), typ, boxes[t - 1], PBC, RCUT, R, T, PAIRS, DELTA)
        V = RK.box_volume(boxes[t - 1])
        counts += c
        amb += a
        cv += c * V
        av += a * V
    share = amb[0].sum() / counts[0].sum()
    print("\n[expected %s %s] %d samples, %d ordered pairs counted, ambiguous bin entries %d for delta = %.2e A (share %.1e)"
          % (tier, ens, len(steps), counts[0].sum(), amb[0].sum(), DELTA, share))
    assert share <= 1e-3, share
    for a in (counts, amb, cv, av):
        a.flags.writeable = False
    return counts, amb, cv, av, steps


def _run(drv, tier, ens, form, calls=None, guard_delay=0, ardf=True, rdf=False, adf=False, msd=False, timing=False):
    from gpumd_amd.nep import ADF, ARDF, RDF, Correlator
    h, typ, x, mass, vel = RC._system(tier)
    n, nsteps = len(typ), NSTEPS[tier]
    calls = tuple(calls or (nsteps,))
    assert sum(calls) == nsteps
    eng = RC._engine(drv, n, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w, d_u = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n), drv.dev(x.copy())
    handles = {}
    if ardf:
        handles["ardf"] = ARDF(eng, RCUT, R, T, INTERVAL, typ, 2, PAIRS)
    if rdf:
        handles["rdf"] = RDF(eng, RR.RC_RDF, RR.BINS, INTERVAL, typ, 2)
    if adf:
        handles["adf"] = ADF(eng, RA.SPECS["triples"], RA.BINS, INTERVAL, typ, 2)
    if msd:
        eng.set_unwrapped(d_u)
        handles["msd"] = Correlator(eng, *RC.MSD)
    for c in handles.values():
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
    out = dict(desc=eng.describe(), st=eng.stats(), got={k: c.read() for k, c in handles.items()}, x=drv.host(d_x), v=drv.host(d_v))
    for c in handles.values():
        eng.detach(c)
        c.close()
    return out


def _compare(tag, tier, ens, got):
    counts, vsum, ns = got
    exp, amb, cv, av, steps = _expected(tier, ens)
    _, _, rebuild_steps, _, strain_tol = RR._frames(tier, ens)
    inside = [r for r in rebuild_steps if 1 < r <= NSTEPS[tier]]
    assert inside and any(min(steps) < r <= max(steps) for r in inside), (steps, rebuild_steps)
    assert ns == len(steps), (ns, len(steps))
    dev = np.abs(counts.astype(np.int64) - exp)
    print("\n[%s] samples %d, ordered pairs %d (expected %d), bins that differ %d, largest |d count| %d, ambiguous allowed %d"
          % (tag, ns, counts[0].sum(), exp[0].sum(), int((dev > 0).sum()), int(dev.max()), int(amb.sum())))
    assert exp[0].sum() > 0 and (dev <= amb).all(), (int(dev.max()), np.argwhere(dev > amb)[:5])
    vdev = np.abs(vsum - cv)
    assert (vdev <= max(strain_tol, 4 * 2.0 ** -52 * len(steps)) * cv + av).all(), float((vdev / np.maximum(cv, 1e-300)).max())


def _nve(drv, tier, form, calls=None):
    out = _run(drv, tier, "nve", form, calls=calls)
    _compare("%s nve %s calls=%s" % (tier, form, calls), tier, "nve", out["got"]["ardf"])
    assert (SCATTER in out["desc"]) == (form == "scatter"), out["desc"]
    assert out["st"].num_rebuild == RR._frames(tier, "nve")[3]


def _together(drv, tier, form):
    """ARDF + RDF + ADF + MSD attached together give what each gives alone, bit for bit"""
    both = _run(drv, tier, "nve", form, rdf=True, adf=True, msd=True)
    _compare("%s nve %s all four" % (tier, form), tier, "nve", both["got"]["ardf"])
    alone = {"ardf": _run(drv, tier, "nve", form), "rdf": _run(drv, tier, "nve", form, ardf=False, rdf=True),
             "adf": _run(drv, tier, "nve", form, ardf=False, adf=True), "msd": _run(drv, tier, "nve", form, ardf=False, msd=True)}
    for k, one in alone.items():
        for a, b in zip(both["got"][k], one["got"][k]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), k
        assert np.array_equal(both["x"], one["x"]) and np.array_equal(both["v"], one["v"])


def _keeps_the_deferred_kick(drv, tier, form, count_launches):
    """a sample reads positions only: the trajectory is bit-identical to the run with nothing attached and (GPU tier: the launch
    counters of nepmi_engine_stats) a 16-step NVE run makes 27 integrator passes with and without the handle"""
    plain = _run(drv, tier, "nve", form, ardf=False, timing=count_launches)
    with_h = _run(drv, tier, "nve", form, timing=count_launches)
    assert np.array_equal(plain["x"], with_h["x"]) and np.array_equal(plain["v"], with_h["v"])
    if count_launches:
        a, b = (int(r["st"].launches[VV_SLOT]) for r in (plain, with_h))
        print("\n[%s nve %s] integrator passes: nothing attached %d, ARDF attached %d" % (tier, form, a, b))
        assert a == b == 27, (a, b)


def _small_box(drv):
    """the loop that steps on the caller's arrays: the 250-atom PbTe cell, 600 K, 1 fs, 6 steps, rc = 6 A, interval 2"""
    from gpumd_amd.nep import ARDF
    fr = H.read_xyz_frames(H.golden("PbTe", "model.xyz"))[0]
    orc = H.Oracle(NEP)
    typ = H.types_from_species(fr["species"], orc.symbols)
    n, h, dt, nsteps, rc = fr["n"], np.asarray(fr["h"], dtype=np.float64), 1.0 / H.TIME_UNIT, 6, 6.0
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 600.0, seed=8)
    x = H.oracle_apply_pbc(h, H.soa(fr["pos"]))
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt, compute=lambda xx: orc.compute(typ, h, xx, precision=32, path=-1))
    exp = np.zeros((1 + len(PAIRS), R, T), dtype=np.int64)
    amb = np.zeros_like(exp)
    for s in range(nsteps):
        loop.run("nve", 1)
        if (s + 1) % INTERVAL == 0:
            c, a = expected_counts(loop.x.reshape(3, -1), typ, h, PBC, rc, R, T, PAIRS, DELTA)
            exp += c
            amb += a
    assert amb[0].sum() <= 1e-3 * exp[0].sum()
    eng = drv.engine(drv.model(NEP), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    r = ARDF(eng, rc, R, T, INTERVAL, typ, 2, PAIRS)
    r.attach()
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    eng.run_nve(h, d_t, d_m, dt, 2, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    eng.run_nve(h, d_t, d_m, dt, 4, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    counts, vsum, ns = r.read()
    r.close()
    dev = np.abs(counts.astype(np.int64) - exp)
    print("\n[%s small box] samples %d pairs %d, largest |d count| %d, ambiguous %d" % (drv.name, ns, exp[0].sum(), dev.max(), amb.sum()))
    assert ns == nsteps // INTERVAL and exp[0].sum() > 0
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
    _compare("gpu npt_ber", "gpu", "npt", out["got"]["ardf"])
    assert out["st"].num_rebuild == RR._frames("gpu", "npt")[3]


@pytest.mark.gpu
def test_guard_band_trip_inside_the_run_samples_once_on_gpu(gpu):
    """scatter form, the guard band narrowed from the 6th force assembly on: that step freezes, the lists are rebuilt and it is
    re-run in the gather form; 16 steps at interval 2 are 8 samples, not 9"""
    out = _run(gpu, "gpu", "nve", "scatter", guard_delay=6)
    assert SCATTER not in out["desc"] and out["st"].discarded_steps >= 1
    assert out["got"]["ardf"][2] == 8
    _compare("gpu nve guard-band trip", "gpu", "nve", out["got"]["ardf"])


@pytest.mark.gpu
def test_small_box_loop_on_gpu(gpu):
    _small_box(gpu)


@pytest.mark.gpu
def test_all_four_together_on_gpu(gpu):
    _together(gpu, "gpu", "gather")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_ardf_sample_does_not_end_the_deferred_kick_on_gpu(gpu, form):
    _keeps_the_deferred_kick(gpu, "gpu", form, True)


@pytest.mark.parametrize("calls", [(20,), (7, 13)])
def test_nve_on_emulator(emu, calls):
    _nve(emu, "emu", "gather", calls)


def test_small_box_loop_on_emulator(emu):
    _small_box(emu)


def test_all_four_together_on_emulator(emu):
    _together(emu, "emu", "gather")


def test_ardf_sample_does_not_end_the_deferred_kick_on_emulator(emu):
    _keeps_the_deferred_kick(emu, "emu", "gather", False)
