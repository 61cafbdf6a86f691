"""Orientational-order handles sampled inside the run loops (Engine::run_md and the small-box loop with nepmi_orient_attach) against
the numpy restatement (test_orient_kernels.restate: all pairs, minimum image, the member rules, Y_lm from the reference's formulas)
on the frames of the oracle's own trajectory at the sample steps.

Systems, oracle frames, temperature, time step, DELTA and the interval of 2 are those of test_run_rdf.py / test_run_adf.py: a list
rebuild lies strictly inside the run with a sample on either side, so the samples come from two internal orders and steps enqueued
behind the freeze word are replayed -- a sample taken twice or lost shows in `sum` and in the counter.
Four handles: `cutoff 3.95` (between PbTe's first shell at 3.29 A and its second at 4.65 A) and `nnn 6`, degrees 4 6, each with and
without `average`.

Ambiguous atoms.  The engine's positions agree with the oracle's within 1e-6 A per coordinate, so a bond within delta = DELTA.  An
atom is ambiguous if a neighbour lies within delta of rc, in mode nnn also if its k-th and (k+1)-th distances differ by less than
2 delta, with `average` also if a member of it is.  Asserted first: they are at most 1e-2 of all atoms.  For the others nn is equal
and |d q_l(i)| <= sqrt(l (l + 1)) delta mean_j(1 / d_ij) (the angular gradient: sum_m |grad Y_lm|^2 = l (l + 1) (2l + 1) / 4 pi);
with `average` the bound is the mean of that over i and its members.  `sum` equals the sum of the per-step expectations within
the summed bounds, for the atoms ambiguous at no sample step."""
import functools
import math

import numpy as np
import pytest

import helpers as H
import test_orient_kernels as OK
import test_run_adf as RA
import test_run_corr as RC
import test_run_npt_ber as NPT
import test_run_rdf as RR

NEP, DT, NSTEPS, SCATTER, VV_SLOT = RC.NEP, RC.DT, RC.NSTEPS, RC.SCATTER, RC.VV_SLOT
INTERVAL, DELTA, PBC = 2, RR.DELTA, (1, 1, 1)
DEGREES = [4, 6]
RC_ORIENT = 3.95
SPECS = [("cutoff", RC_ORIENT, False), ("cutoff", RC_ORIENT, True), ("nnn", 6, False), ("nnn", 6, True)]


def _expect_frame(pos, h9):
    """-> per spec: (ql [n, 2], nn, ambiguous, bound [n, 2])"""
    out, pre = [], {}
    for mode, value, average in SPECS:
        if mode not in pre:
            pre[mode] = OK.bonds(pos, h9, PBC, mode, value, rc_search=6.0, delta=DELTA)
        ref = OK.restate(pos, h9, PBC, mode, value, DEGREES, average, delta=DELTA, pre=pre[mode])
        b = DELTA * ref["minv"]
        if average:
            b = (b + np.bincount(ref["ci"], weights=b[ref["cj"]], minlength=len(b))) / (ref["nn"] + 1.0)
        bound = b[:, None] * np.array([math.sqrt(l * (l + 1.0)) for l in DEGREES])[None, :]
        out.append((ref["cols"], ref["nn"], ref["amb"], bound))
    return out


@functools.lru_cache(maxsize=None)
def _expected(tier, ens):
    """-> per spec: dict(last, nn, amb_last, bound_last, sum, amb_any, bound_sum), the 1-based sample steps"""
    frames, boxes, _, _, _ = RR._frames(tier, ens)
    steps = list(range(INTERVAL, NSTEPS[tier] + 1, INTERVAL))
    acc = None
    for t in steps:
        per = _expect_frame(np.ascontiguousarray(frames[t - 1].reshape(3, -1)), boxes[t - 1])
        if acc is None:
            acc = [dict(sum=np.zeros_like(c), amb_any=np.zeros_like(a), bound_sum=np.zeros_like(b)) for c, _, a, b in per]
        for e, (c, nn, a, b) in zip(acc, per):
            e["sum"] = e["sum"] + c
            e["amb_any"] = e["amb_any"] | a
            e["bound_sum"] = e["bound_sum"] + b
            e.update(last=c, nn=nn, amb_last=a, bound_last=b)
    for e, spec in zip(acc, SPECS):
        share = e["amb_any"].mean()
        print("\n[expected %s %s %s] %d samples, ambiguous atoms %d of %d for delta = %.2e A, mean nn %.2f"
              % (tier, ens, spec, len(steps), e["amb_any"].sum(), len(e["nn"]), DELTA, e["nn"].mean()))
        assert share <= 1e-2, share
        for a in e.values():
            a.setflags(write=False)
    return acc, steps


def _run(drv, tier, ens, form, calls=None, guard_delay=0, orient=True, others=False, timing=False):
    from gpumd_amd.nep import ADF, RDF, Correlator, OrientOrder
    h, typ, x, mass, vel = RC._system(tier)
    n, nsteps = len(typ), NSTEPS[tier]
    calls = tuple(calls or (nsteps,))
    assert sum(calls) == nsteps
    eng = RC._engine(drv, n, form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w, d_u = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n), drv.dev(x.copy())
    handles = [OrientOrder(eng, m, v, DEGREES, average=a, interval=INTERVAL) for m, v, a in SPECS] if orient else []
    if others:
        handles.append(RDF(eng, RR.RC_RDF, RR.BINS, INTERVAL, typ, 2))
        handles.append(ADF(eng, RA.SPECS["global"], RA.BINS, INTERVAL, typ, 2))
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


def _compare(tag, tier, ens, out):
    acc, steps = _expected(tier, ens)
    rebuild_steps = RR._frames(tier, ens)[2]
    inside = [r for r in rebuild_steps if 1 < r <= NSTEPS[tier]]
    assert inside and any(min(steps) < r <= max(steps) for r in inside), (steps, rebuild_steps)
    for spec, e, (last, total, nn, ns) in zip(SPECS, acc, out["got"][:len(SPECS)]):
        assert ns == len(steps), (spec, ns, len(steps))
        ok = ~e["amb_last"]
        assert np.array_equal(nn[ok], e["nn"][ok]), (spec, np.flatnonzero(nn != e["nn"])[:5])
        dev = np.abs(last - e["last"])[ok]
        used = float((dev / e["bound_last"][ok]).max())
        assert (dev <= e["bound_last"][ok]).all(), (spec, float(dev.max()), used)
        oks = ~e["amb_any"]
        devs = np.abs(total - e["sum"])[oks]
        useds = float((devs / e["bound_sum"][oks]).max())
        assert (devs <= e["bound_sum"][oks]).all(), (spec, float(devs.max()), useds)
        assert e["nn"].mean() > 4 and e["last"].max() > 0.3
        print("\n[%s %s] samples %d, atoms compared %d of %d; last: largest |d ql| %.2e (%.2f of its bound); sum: %.2e (%.2f)"
              % (tag, spec, ns, ok.sum(), len(ok), dev.max(), used, devs.max(), useds))


def _nve(drv, tier, form, calls=None):
    out = _run(drv, tier, "nve", form, calls=calls)
    _compare("%s nve %s calls=%s" % (tier, form, calls), tier, "nve", out)
    assert (SCATTER in out["desc"]) == (form == "scatter"), out["desc"]
    assert out["st"].num_rebuild == RR._frames(tier, "nve")[3]


def _together(drv, tier, form):
    """the handles beside RDF + ADF + MSD: equal to the handles alone, bit for bit (no floating-point atomics, a fixed order)"""
    alone = _run(drv, tier, "nve", form)
    out = _run(drv, tier, "nve", form, others=True)
    _compare("%s nve %s beside rdf + adf + msd" % (tier, form), tier, "nve", out)
    for k in range(len(SPECS)):
        for a, b in zip(out["got"][k][:3], alone["got"][k][:3]):
            assert np.array_equal(a, b)
        assert out["got"][k][3] == alone["got"][k][3]
    assert np.array_equal(out["x"], alone["x"])


def _keeps_the_deferred_kick(drv, tier, form, count_launches):
    """a sample reads positions only: the trajectory is bit-identical to the run with nothing attached and (GPU tier: the launch
    counters of nepmi_engine_stats) the loop makes the same number of integrator passes: 27 in 16 steps"""
    plain = _run(drv, tier, "nve", form, orient=False, timing=count_launches)
    att = _run(drv, tier, "nve", form, timing=count_launches)
    assert np.array_equal(plain["x"], att["x"]) and np.array_equal(plain["v"], att["v"])
    if count_launches:
        a, b = (int(r["st"].launches[VV_SLOT]) for r in (plain, att))
        print("\n[%s nve %s] integrator passes: nothing attached %d, orientational order attached %d" % (tier, form, a, b))
        assert a == b == 27, (a, b)


def _small_box(drv):
    """the loop that steps on the caller's arrays: the 250-atom PbTe cell (19 A thick), 600 K, 1 fs, 6 steps, interval 2; oracle:
    helpers.OracleLoop on the branch the oracle picks itself"""
    from gpumd_amd.nep import OrientOrder
    fr = H.read_xyz_frames(H.golden("PbTe", "model.xyz"))[0]
    orc = H.Oracle(NEP)
    typ = H.types_from_species(fr["species"], orc.symbols)
    n, h, dt, nsteps = fr["n"], np.asarray(fr["h"], dtype=np.float64), 1.0 / H.TIME_UNIT, 6
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 600.0, seed=8)
    x = H.oracle_apply_pbc(h, H.soa(fr["pos"]))
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt, compute=lambda xx: orc.compute(typ, h, xx, precision=32, path=-1))
    sums = bsum = amb = per = None
    for s in range(nsteps):
        loop.run("nve", 1)
        if (s + 1) % INTERVAL == 0:
            per = _expect_frame(np.ascontiguousarray(loop.x.reshape(3, -1)), h)
            if sums is None:
                sums, bsum, amb = [0.0 * c for c, _, _, _ in per], [0.0 * b for _, _, _, b in per], [a & False for _, _, a, _ in per]
            for k, (c, _, a, b) in enumerate(per):
                sums[k], bsum[k], amb[k] = sums[k] + c, bsum[k] + b, amb[k] | a
    eng = drv.engine(drv.model(NEP), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    handles = [OrientOrder(eng, m, v, DEGREES, average=a, interval=INTERVAL) for m, v, a in SPECS]
    for o in handles:
        eng.attach(o)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    eng.run_nve(h, d_t, d_m, dt, 2, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    eng.run_nve(h, d_t, d_m, dt, 4, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    for k, (spec, o) in enumerate(zip(SPECS, handles)):
        last, total, nn, ns = o.read()
        o.close()
        assert amb[k].mean() <= 1e-2
        ok = ~amb[k]
        assert ns == nsteps // INTERVAL and np.array_equal(nn[ok], per[k][1][ok]) and per[k][1].mean() > 4
        dev, devs = np.abs(last - per[k][0])[ok], np.abs(total - sums[k])[ok]
        print("\n[%s small box %s] samples %d, largest |d ql| %.2e (bound %.2e), of the sum %.2e"
              % (drv.name, spec, ns, dev.max(), per[k][3][ok].max(), devs.max()))
        assert (dev <= per[k][3][ok]).all() and (devs <= bsum[k][ok]).all()


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
    _compare("gpu npt_ber", "gpu", "npt", out)
    assert out["st"].num_rebuild == RR._frames("gpu", "npt")[3]


@pytest.mark.gpu
def test_guard_band_trip_inside_the_run_samples_once_on_gpu(gpu):
    """scatter form, the guard band narrowed from the 6th force assembly on: that step freezes, the lists are rebuilt and it is
    re-run in the gather form; 16 steps at interval 2 are 8 samples, not 9"""
    out = _run(gpu, "gpu", "nve", "scatter", guard_delay=6)
    assert SCATTER not in out["desc"] and out["st"].discarded_steps >= 1
    assert all(g[3] == 8 for g in out["got"])
    _compare("gpu nve guard-band trip", "gpu", "nve", out)


@pytest.mark.gpu
def test_small_box_loop_on_gpu(gpu):
    _small_box(gpu)


@pytest.mark.gpu
def test_beside_rdf_adf_and_msd_on_gpu(gpu):
    _together(gpu, "gpu", "gather")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_sample_does_not_end_the_deferred_kick_on_gpu(gpu, form):
    _keeps_the_deferred_kick(gpu, "gpu", form, True)


@pytest.mark.parametrize("calls", [(20,), (7, 13)])
def test_nve_on_emulator(emu, calls):
    _nve(emu, "emu", "gather", calls)


def test_small_box_loop_on_emulator(emu):
    _small_box(emu)


def test_beside_rdf_adf_and_msd_on_emulator(emu):
    _together(emu, "emu", "gather")


def test_sample_does_not_end_the_deferred_kick_on_emulator(emu):
    _keeps_the_deferred_kick(emu, "emu", "gather", False)
