"""nepmi_run_npt_ber (`ensemble npt_ber`: Ensemble_BER with type 11, ensemble_ber.cu:88-176, :195-285) against an oracle NPT
stepper composed from the oracle's pieces, on trajectories where the box changes on EVERY step and the Verlet lists must survive
that: the engine re-metrics itself on the host (cells, lists and window tables stay) and rebuilds only when the skin rule -- with
the rebuild-time positions kept in the old metric -- fires.  The rebuild count must equal the oracle's step for step, with at
least one rebuild and at least one kept-list step inside the run.

The oracle stepper (NptOracle below; helpers.OracleLoop closes over a fixed box), per step: nepo_velocity_verlet(first),
oracle_apply_pbc(h, x), oracle_skin_moved(h, x, x_rebuild) with the CURRENT h, Oracle.compute(typ, h, x, precision=32, path=0),
nepo_velocity_verlet(second), oracle_thermo(volume(h), ...), the Berendsen velocity factor, then the box and position update in
numpy written from cpu_pressure_isotropic / _orthogonal / _triclinic and gpu_pressure_* (same expressions, same order, the
literal 0.3333333333333333).  Box rows are the box AFTER the step's scaling (what thermo.out prints next to the row).

Systems (hot: 6000 K Maxwell velocities, 2 fs steps, PbTe nep.txt, `npt_ber 6000 5000 20 ...`, tau_p = 100):
  orthogonal  H.rocksalt_orthogonal((7, 8, 7)), 3,136 atoms, both tiers: isotropic (0 GPa, 40 GPa) and three components
              (targets 0 0.5 1 GPa, moduli 40 50 60 GPa); pressure 5.6-6.5 GPa, mu - 1 about 5e-4 per step
  triclinic   H.pbte_supercell((3, 3, 3)), 6,750 atoms on the GPU (12 cells per direction: the window kernels run),
              (2, 2, 2) on the emulator: six components with shear targets 0 0 0 0.5 -0.5 1.0 GPa so that the off-diagonal mu show

Tolerances: those of test_run_loop_oracle._case (T, U rtol 1e-6; stress rtol 1e-4 / atol 1e-6; velocities 1e-6; final forces,
energies, virials as in the header of parity_cases.py).  Positions are compared in FRACTIONAL coordinates multiplied by the
oracle's final box, within 1e-6 A, so that a box deviation is not counted twice.  Box rows and the final h: the stress tolerance
propagated through mu, strain <= steps x max_i p_coupling_i x (1e-4 max|p| + 1e-6) with max|p| from the oracle's own rows, applied
to every component as |dh| <= strain x max|h|; the measured deviation is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H

SCATTER = "lds_scatter_of_own_halves"
NEP = H.golden("PbTe", "nep.txt")
T0, DT = 6000.0, 2.0 / H.TIME_UNIT
T1, T2, TC = 6000.0, 5000.0, 20.0
GPA = 1.602177e+2  # PRESSURE_UNIT_CONVERSION, natural units -> GPa
TAU_P = 100.0
_dp = C.POINTER(C.c_double)


def _barostat(kind):
    """-> (p_target, p_coupling) in natural units like Integrate::parse_ensemble leaves them (integrate.cu:709-714, :1152-1153)"""
    gpa, mod = {"iso": ([0.0], [40.0]), "ortho": ([0.0, 0.5, 1.0], [40.0, 50.0, 60.0]),
                "tri": ([0.0, 0.0, 0.0, 0.5, -0.5, 1.0], [40.0] * 6)}[kind]
    pc = np.array([1.0 / (TAU_P * 3.0 * m) for m in mod]) * GPA
    return np.array(gpa) / GPA, pc


@functools.lru_cache(maxsize=None)
def _system(name):
    if name == "ortho":
        h, typ, x = H.rocksalt_orthogonal((7, 8, 7), rattle=0.02, seed=9)
    else:
        h, typ, x = H.pbte_supercell({"tri3": (3, 3, 3), "tri2": (2, 2, 2)}[name], rattle=0.02, seed=31)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    vel = H.maxwell_velocities(mass, T0, seed=5)
    return np.array(h, dtype=np.float64).reshape(9), typ, x, mass, vel


def _sysname(kind, tier):
    return "ortho" if kind in ("iso", "ortho") else ("tri3" if tier == "gpu" else "tri2")


NSTEPS = {"ortho": 16, "tri3": 16, "tri2": 20}


class NptOracle:
    """Run::perform_a_run for `ensemble npt_ber`, one Oracle.compute per step; the state (x, v, f, pe, w, h, the positions of the
    last list rebuild) is carried between calls of run()"""

    def __init__(self, orc, typ, h, x, vel, mass, dt):
        self.L, self.orc = H.oracle_lib(), orc
        self.typ, self.mass, self.dt, self.n = typ, np.ascontiguousarray(mass, dtype=np.float64), float(dt), len(typ)
        self.h = np.array(h, dtype=np.float64).reshape(9)
        self.x, self.v = np.array(x, dtype=np.float64), np.array(vel, dtype=np.float64)
        self.pe, self.f, self.w = orc.compute(typ, self.h, self.x, precision=32, path=0)  # Run: initial force before the loop
        self.x_rebuild, self.rebuilds, self.rebuild_steps, self.steps_done = self.x.copy(), 1, [], 0
        self.mu_offdiag = 0.0

    def _vv(self, first):
        p = lambda a: a.ctypes.data_as(_dp)  # noqa: E731
        self.L.nepo_velocity_verlet(1 if first else 0, self.n, self.dt, p(self.mass), p(self.f), p(self.x), p(self.v))

    def _scale(self, kind, p0, pc, th):
        """ensemble_ber.cu:138-176 (+ :88-136 without deform) and npt_utilities.cuh: h and x after the step"""
        p, h, n = th[2:8], self.h, self.n
        x, y, z = self.x[:n].copy(), self.x[n:2 * n].copy(), self.x[2 * n:].copy()
        if kind == "iso":
            s = 1.0 - pc[0] * (p0[0] - (p[0] + p[1] + p[2]) * 0.3333333333333333)
            h[0] *= s; h[4] *= s; h[8] *= s  # noqa: E702
            x *= s; y *= s; z *= s  # noqa: E702
        elif kind == "ortho":
            s = [1.0 - pc[d] * (p0[d] - p[d]) for d in range(3)]  # (all directions periodic here)
            h[0] *= s[0]; h[4] *= s[1]; h[8] *= s[2]  # noqa: E702
            x *= s[0]; y *= s[1]; z *= s[2]  # noqa: E702
        else:
            mu = np.zeros(9)
            mu[0] = 1.0 - pc[0] * (p0[0] - p[0])
            mu[4] = 1.0 - pc[1] * (p0[1] - p[1])
            mu[8] = 1.0 - pc[2] * (p0[2] - p[2])
            mu[3] = mu[1] = -pc[5] * (p0[5] - p[3])  # xy  (thermo order: xx yy zz xy xz yz)
            mu[6] = mu[2] = -pc[4] * (p0[4] - p[4])  # xz
            mu[7] = mu[5] = -pc[3] * (p0[3] - p[5])  # yz
            h_old = h.copy()
            for r in range(3):
                for c in range(3):
                    tmp = 0.0
                    for k in range(3):
                        tmp += mu[r * 3 + k] * h_old[k * 3 + c]
                    h[r * 3 + c] = tmp
            x, y, z = (mu[0] * x + mu[1] * y + mu[2] * z, mu[3] * x + mu[4] * y + mu[5] * z, mu[6] * x + mu[7] * y + mu[8] * z)
            self.mu_offdiag = max(self.mu_offdiag, float(np.abs(mu[[1, 2, 5]]).max()))
        self.x = np.concatenate([x, y, z])

    def run(self, kind, nsteps, p0, pc):
        rows, boxes = [], []
        for step in range(nsteps):
            target = T1 + (T2 - T1) * (step / nsteps)
            self._vv(True)
            self.x = H.oracle_apply_pbc(self.h, self.x)
            if H.oracle_skin_moved(self.h, self.x, self.x_rebuild):
                self.x_rebuild = self.x.copy()
                self.rebuilds += 1
                self.rebuild_steps.append(self.steps_done + 1)
            self.pe, self.f, self.w = self.orc.compute(self.typ, self.h, self.x, precision=32, path=0)
            self._vv(False)
            vol = abs(np.linalg.det(self.h.reshape(3, 3)))
            th = H.oracle_thermo(vol, self.mass, self.pe, self.v, self.w)
            self.v *= np.sqrt(1.0 + (1.0 / TC) * (target / th[0] - 1.0))
            self._scale(kind, p0, pc, th)
            self.steps_done += 1
            rows.append(th)
            boxes.append(self.h.copy())
        return np.array(rows), np.array(boxes)


@functools.lru_cache(maxsize=None)
def _reference(sysname, kind, calls):
    import time
    h, typ, x, mass, vel = _system(sysname)
    p0, pc = _barostat(kind)
    t0 = time.time()
    loop = NptOracle(H.Oracle(NEP), typ, h, x, vel, mass, DT)
    out = [loop.run(kind, k, p0, pc) for k in calls]
    ref = dict(rows=np.concatenate([o[0] for o in out]), boxes=np.concatenate([o[1] for o in out]), x=loop.x, v=loop.v, pe=loop.pe,
               f=loop.f, w=loop.w, h=loop.h.copy(), rebuilds=loop.rebuilds, rebuild_steps=tuple(loop.rebuild_steps),
               mu_offdiag=loop.mu_offdiag)
    print("\n[oracle npt %s %s %s] %.1f s, list rebuilds (initial one included) %d at steps %s, pressure %.2f..%.2f GPa"
          % (sysname, kind, calls, time.time() - t0, ref["rebuilds"], ref["rebuild_steps"],
             ref["rows"][:, 2:5].mean(axis=1).min() * GPA, ref["rows"][:, 2:5].mean(axis=1).max() * GPA))
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


def _start(drv, sysname, form):
    h, typ, x, mass, vel = _system(sysname)
    n = len(typ)
    eng = _engine(drv, n, form)
    st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
    eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])  # Run: initial force before the loop
    return eng, st, h.copy()


def _case(drv, tier, kind, form, thermo_every, calls=None):
    sysname = _sysname(kind, tier)
    h0, typ, x, mass, vel = _system(sysname)
    n = len(typ)
    calls = tuple(calls or (NSTEPS[sysname],))
    total = sum(calls)
    ref = _reference(sysname, kind, calls)
    assert ref["rebuilds"] - 1 >= 1, "no list rebuild inside the oracle's run: raise the step count"
    assert ref["rebuilds"] - 1 < total, "no step on kept lists inside the oracle's run"
    if kind == "tri":
        assert ref["mu_offdiag"] > 1e-5, ref["mu_offdiag"]  # the shear targets make the off-diagonal mu visible
    p0, pc = _barostat(kind)

    eng, st, box = _start(drv, sysname, form)
    rows, boxes, pick, done = [], [], [], 0
    for k in calls:
        th, bx = eng.run_npt_ber(box, st["t"], st["m"], DT, k, T1, T2, TC, p0, pc, st["x"], st["v"], st["pe"], st["f"], st["w"],
                                 thermo_every=thermo_every)
        assert th.shape == (k // thermo_every, 8) and bx.shape == (k // thermo_every, 9)
        rows.append(th)
        boxes.append(bx)
        pick += [done + thermo_every * (j + 1) - 1 for j in range(k // thermo_every)]
        done += k
    rows, boxes = np.concatenate(rows), np.concatenate(boxes)
    rows_ref, boxes_ref = ref["rows"][pick], ref["boxes"][pick]
    desc, stt = eng.describe(), eng.stats()
    xs, vs, pe, f, w = (drv.host(st[a]) for a in ("x", "v", "pe", "f", "w"))

    Hr, He = ref["h"].reshape(3, 3), box.reshape(3, 3)
    frac = np.linalg.solve(He, xs.reshape(3, n)) - np.linalg.solve(Hr, ref["x"].reshape(3, n))
    frac -= np.rint(frac)
    strain_tol = total * pc.max() * (1e-4 * np.abs(ref["rows"][:, 2:]).max() + 1e-6)
    hscale = np.abs(ref["h"]).max()
    dev = dict(pos=np.abs(Hr @ frac).max(), vel=np.abs(vs - ref["v"]).max(),
               f=(np.abs(f - ref["f"]) - 1e-4 * np.abs(ref["f"])).max(), w=(np.abs(w - ref["w"]) - 1e-4 * np.abs(ref["w"])).max(),
               box_rows=np.abs(boxes - boxes_ref).max() / hscale, h=np.abs(box - ref["h"]).max() / hscale)
    print("\n[%s npt_ber %s %s thermo_every=%d calls=%s] rebuilds engine %d oracle %d (initial one included; oracle at steps %s)\n"
          "  max deviation: positions (fractional x oracle box) %.2e A, velocities %.2e, T rel %.2e, U rel %.2e, stress abs %.2e\n"
          "  box rows %.2e, final h %.2e (relative to max|h|; tolerance %.2e); total strain of the run %.2e\n"
          "  final state, excess over the relative part: forces %.2e eV/A, virials %.2e eV\n  %s"
          % (tier, kind, form, thermo_every, calls, stt.num_rebuild, ref["rebuilds"], ref["rebuild_steps"], dev["pos"], dev["vel"],
             np.abs(rows[:, 0] / rows_ref[:, 0] - 1.0).max(), np.abs(rows[:, 1] / rows_ref[:, 1] - 1.0).max(),
             np.abs(rows[:, 2:] - rows_ref[:, 2:]).max(), dev["box_rows"], dev["h"], strain_tol,
             np.abs(ref["h"] - h0).max() / hscale, dev["f"], dev["w"], desc))

    assert (SCATTER in desc) == (form == "scatter"), desc
    assert stt.num_rebuild == ref["rebuilds"], (stt.num_rebuild, ref["rebuilds"])
    assert np.isfinite(rows).all() and len(rows) >= 1
    np.testing.assert_allclose(rows[:, 0], rows_ref[:, 0], rtol=1e-6)
    np.testing.assert_allclose(rows[:, 1], rows_ref[:, 1], rtol=1e-6)
    np.testing.assert_allclose(rows[:, 2:], rows_ref[:, 2:], rtol=1e-4, atol=1e-6)
    assert np.abs(ref["h"] - h0).max() / hscale > 10 * strain_tol  # the box really moves, far beyond what the tolerance hides
    assert dev["box_rows"] <= strain_tol and dev["h"] <= strain_tol, dev
    assert np.array_equal(boxes[-1], box) if total % thermo_every == 0 and len(calls) == 1 else True
    assert dev["pos"] < 1e-6 and dev["vel"] < 1e-6, dev
    assert dev["f"] <= 2e-5, dev
    np.testing.assert_allclose(pe, ref["pe"], rtol=1e-5, atol=2e-5)
    assert dev["w"] <= 1e-4, dev


def _limit(drv, tier, other):
    """p_coupling = 0: the loop is run_nve (T_coup = 1e300) / run_nvt_ber (T_coup = 20) of the same library: their thermo rows
    within the tolerances above, the box unchanged bit for bit"""
    h0, typ, x, mass, vel = _system("ortho")
    nsteps, tc = NSTEPS["ortho"], (1e300 if other == "nve" else TC)
    eng, st, box = _start(drv, "ortho", "gather")
    th, bx = eng.run_npt_ber(box, st["t"], st["m"], DT, nsteps, T1, T2, tc, [0.0], [0.0], st["x"], st["v"], st["pe"], st["f"], st["w"],
                             thermo_every=1)
    eng2, s2, _ = _start(drv, "ortho", "gather")
    args = (s2["x"], s2["v"], s2["pe"], s2["f"], s2["w"])
    if other == "nve":
        th2 = eng2.run_nve(h0, s2["t"], s2["m"], DT, nsteps, *args, thermo_every=1)
    else:
        th2 = eng2.run_nvt_ber(h0, s2["t"], s2["m"], DT, nsteps, T1, T2, TC, *args, thermo_every=1)
    print("\n[%s npt_ber with p_coupling = 0 against run_%s] max rel T %.2e, U %.2e, stress abs %.2e; rebuilds %d / %d"
          % (tier, other, np.abs(th[:, 0] / th2[:, 0] - 1).max(), np.abs(th[:, 1] / th2[:, 1] - 1).max(),
             np.abs(th[:, 2:] - th2[:, 2:]).max(), eng.stats().num_rebuild, eng2.stats().num_rebuild))
    assert np.array_equal(box, h0) and np.array_equal(bx, np.tile(h0, (nsteps, 1)))
    assert eng.stats().num_rebuild == eng2.stats().num_rebuild >= 2
    np.testing.assert_allclose(th[:, 0], th2[:, 0], rtol=1e-6)
    np.testing.assert_allclose(th[:, 1], th2[:, 1], rtol=1e-6)
    np.testing.assert_allclose(th[:, 2:], th2[:, 2:], rtol=1e-4, atol=1e-6)
    assert np.abs(drv.host(st["x"]) - drv.host(s2["x"])).max() < 1e-6 and np.abs(drv.host(st["v"]) - drv.host(s2["v"])).max() < 1e-6


def _refusals(drv):
    from gpumd_amd._capi import NepmiError
    cases = []
    for sysname, pbc, npc, msg in (("tri2", (1, 1, 1), 3, "Cannot use triclinic box with only 3 target pressure components."),
                                   ("tri2", (1, 1, 1), 1, "Cannot use triclinic box with only 1 target pressure component."),
                                   ("ortho", (1, 1, 0), 1, "Cannot use isotropic pressure with non-periodic boundary in any direction."),
                                   ("tri2", (1, 0, 1), 6, "Cannot use 6 pressure components with non-periodic boundary in any direction.")):
        h, typ, x, mass, vel = _system(sysname)
        n = len(typ)
        eng = drv.engine(drv.model(NEP), n, pbc=pbc)
        a = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
        box = h.copy()
        with pytest.raises(NepmiError) as ei:
            eng.run_npt_ber(box, a["t"], a["m"], DT, 2, T1, T2, TC, [0.0] * npc, [1e-3] * npc, a["x"], a["v"], a["pe"], a["f"], a["w"])
        assert ei.value.code == -4 and msg in str(ei.value), (ei.value.code, str(ei.value))
        assert np.array_equal(box, h) and np.array_equal(drv.host(a["x"]), x)  # nothing ran
        cases.append(msg)
    h, typ, x, mass, vel = _system("ortho")
    n = len(typ)
    eng = drv.engine(drv.model(NEP), n)
    a = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
    with pytest.raises(NepmiError) as ei:  # integrate.cu:594-602
        eng.run_npt_ber(h.copy(), a["t"], a["m"], DT, 2, T1, T2, 0.5, [0.0], [1e-3], a["x"], a["v"], a["pe"], a["f"], a["w"])
    assert "Temperature coupling should >= 1." in str(ei.value)
    with pytest.raises(ValueError):
        eng.run_npt_ber(h.copy(), a["t"], a["m"], DT, 2, T1, T2, TC, [0.0, 0.0], [1e-3, 1e-3], a["x"], a["v"], a["pe"], a["f"], a["w"])
    assert len(cases) == 4


def _stepwise_barostat(drv):
    """nepmi_berendsen_pressure, the barostat step for a host that steps by hand: box and positions against numpy"""
    h, typ, x, mass, vel = _system("tri2")
    n = len(typ)
    eng = drv.engine(drv.model(NEP), n)
    p0, pc = _barostat("tri")
    th = np.array([300.0, -1.0, 0.04, 0.035, 0.03, 0.002, -0.001, 0.003])
    loop = NptOracle.__new__(NptOracle)
    loop.h, loop.x, loop.n, loop.mu_offdiag = h.copy(), x.copy(), n, 0.0
    loop._scale("tri", p0, pc, th)
    box, d_x = h.copy(), drv.dev(x)
    eng.berendsen_pressure(box, p0, pc, drv.dev(th), d_x)
    assert np.abs(box - loop.h).max() <= 1e-14 * np.abs(h).max() and not np.array_equal(box, h)
    assert np.abs(drv.host(d_x) - loop.x).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


KINDS = ["iso", "ortho", "tri"]
FORMS = ["gather", "scatter"]


@pytest.mark.gpu
@pytest.mark.parametrize("thermo_every", [1, 5])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_npt_ber_on_gpu(gpu, kind, form, thermo_every):
    _case(gpu, "gpu", kind, form, thermo_every)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_npt_ber_two_calls_on_gpu(gpu, kind, form):
    """7 + 9 steps on one engine: the second call starts from the box and the scaled, not yet wrapped positions the first left"""
    _case(gpu, "gpu", kind, form, 1, calls=(7, 9))


@pytest.mark.gpu
@pytest.mark.parametrize("other", ["nve", "nvt_ber"])
def test_npt_ber_without_barostat_is_the_other_loop_on_gpu(gpu, other):
    _limit(gpu, "gpu", other)


@pytest.mark.gpu
def test_npt_ber_refusals_and_stepwise_barostat_on_gpu(gpu):
    _refusals(gpu)
    _stepwise_barostat(gpu)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU tier: the kernel emulator (gather form)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.parametrize("kind,thermo_every,calls", [("iso", 1, None), ("ortho", 5, None), ("tri", 1, None), ("tri", 5, (9, 11))])
def test_npt_ber_on_emulator(emu, kind, thermo_every, calls):
    _case(emu, "emu", kind, "gather", thermo_every, calls=calls)


@pytest.mark.parametrize("other", ["nve", "nvt_ber"])
def test_npt_ber_without_barostat_is_the_other_loop_on_emulator(emu, other):
    _limit(emu, "emu", other)


def test_npt_ber_refusals_and_stepwise_barostat_on_emulator(emu):
    _refusals(emu)
    _stepwise_barostat(emu)
