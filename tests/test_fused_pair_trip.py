"""GPU tier: the fused angular kernel with its record loops in trips of two records (engine option "angular_pair_trip" = 1, the
default: each lane of an atom's lane pair evaluates the radial part of ONE of the two records and hands the partner that
record's values for the partner's channels) against the one-record loops (option = 0): the same operations on the same
operands in the same order, so every output must be bit-identical -- per-call evaluations (energies, forces, virials, the
exported descriptor and Fp) and 50-step run loops with list rebuilds.

The partial forces f12 have no export of their own: they are compared through what is made of them and of nothing else that
the option touches -- the forces and per-atom virials of the gather form (per-call evaluations: f12 - f21 summed in list order)
and the integer window sums of the scatter form (run loops)."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

FUSED = "partial_forces_in_one_kernel"
TRIPS = "two_record_trips"


@pytest.fixture(scope="module")
def drv():
    return H.GpuDriver()


def _trips_apply(model):
    """shapes with at most four angular channels per lane take the trips (nep_fused.h: kFusedTripMaxChannels)"""
    return (model.info.n_max_angular + 2) // 2 <= 4


def _per_call(drv, model, h, typ, x, trip):
    n = len(typ)
    eng = drv.engine(model, n)
    eng.set_angular_pair_trip(trip)
    _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    d = eng.describe()
    assert FUSED in d and (TRIPS in d) == (bool(trip) and _trips_apply(model)), d
    q = drv.zeros(model.info.dim * n, dtype=np.float32)
    fp = drv.zeros(model.info.dim * n, dtype=np.float32)
    eng.descriptors(q, fp)
    return {"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)}


def _run(drv, model, h, typ, x, mass, temp, trip, nsteps=50, dt_fs=2.0, force_form=None):
    n = len(typ)
    vel = H.maxwell_velocities(mass, temp, seed=4)
    eng = drv.engine(model, n)
    eng.set_angular_pair_trip(trip)
    if force_form is not None:  # (systems below the size the run loops' rule asks for: pin the one-lane scatter form)
        eng.set_win_lanes(1)
        eng.set_force_form(force_form)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    r0 = eng.stats().num_rebuild
    th = eng.run_nve(h, d_t, d_m, dt_fs / H.TIME_UNIT, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=10)
    d = eng.describe()
    assert FUSED in d and (TRIPS in d) == (bool(trip) and _trips_apply(model)), d
    return {"x": drv.host(d_x), "vel": drv.host(d_v), "f": drv.host(d_f), "pe": drv.host(d_pe), "w": drv.host(d_w),
            "th": np.asarray(th)}, eng.stats().num_rebuild - r0, d


def _same(a, b):
    for key in a:
        print("%-4s equal=%s  max|diff|=%.3e" % (key, np.array_equal(a[key], b[key]), np.abs(a[key] - b[key]).max()))
    for key in a:
        assert np.array_equal(a[key], b[key]), (key, np.abs(a[key] - b[key]).max())


def _both(drv, nep, h, typ, x, mass, temp, scatter_expected, force_form=None, nsteps=50, dt_fs=2.0):
    model = drv.model(nep)
    _same(_per_call(drv, model, h, typ, x, 0), _per_call(drv, model, h, typ, x, 1))
    (r0, nb0, d0), (r1, nb1, d1) = (_run(drv, model, h, typ, x, mass, temp, t, nsteps, dt_fs, force_form) for t in (0, 1))
    print("list rebuilds inside the run: %d / %d" % (nb0, nb1))
    assert nb0 >= 1 and nb1 == nb0, (nb0, nb1)
    if scatter_expected:
        assert "lds_scatter_of_own_halves" in d0 and "lds_scatter_of_own_halves" in d1, (d0, d1)
    _same(r0, r1)


def test_pbte_triclinic_250k(drv):
    """250,000 atoms, triclinic: large enough for the run loops' scatter form.  600 K: two list rebuilds inside the 50 steps, and no atom
    of the quarter million gathers more angular neighbours than the model's lists hold (from 1200 K on one does)"""
    h, typ, x = H.pbte_supercell((10, 10, 10), rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    _both(drv, H.golden("PbTe", "nep.txt"), h, typ, x, mass, 600.0, True)


def test_carbon_262k(drv):
    """262,144 atoms of diamond, hot enough for a list rebuild inside 50 steps.  Nine angular channels, five per lane: this shape
    keeps the one-record loops under either value of the option (the trips would add to its scratch), which is what the case pins."""
    h, typ, x = H.diamond((32, 32, 32), 3.57, rattle=0.05, seed=18)
    mass = np.full(len(typ), H.MASS["C"])
    _both(drv, H.golden("C", "nep.txt"), h, typ, x, mass, 12000.0, True)


@pytest.mark.parametrize("kind", ["typewise", "flexible"])
def test_zbl_models(drv, tmp_path, kind):
    """ZBL stays per pair on alternating lanes and must see the same d and 1/d: the universal form with a type-wise outer cutoff and
    the flexible form (ten parameters per type pair), on PbTe"""
    import test_model_variants as V
    nep = V.make_typewise_zbl(tmp_path) if kind == "typewise" else V.make_flexible_zbl(tmp_path)
    h, typ, x = H.pbte_supercell((6, 6, 6), rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    _both(drv, nep, h, typ, x, mass, 1500.0, True, force_form=1)


def _sparse_gas(seed=5, sites=20, spacing=5.0, fill=0.5, jitter=1.4):
    """Half-filled jittered grid in an orthogonal periodic box: no two atoms closer than spacing - 2 jitter = 2.2 A, and between
    none and a handful of neighbours inside the angular cutoff of 4 A."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(sites)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[rng.random(len(g)) < fill]
    pos = (g + 0.5) * spacing + rng.uniform(-jitter, jitter, g.shape)
    L = sites * spacing
    h = np.diag([L, L, L]).reshape(9).astype(np.float64)
    typ = (rng.random(len(pos)) < 0.5).astype(np.int32)
    x = H.oracle_apply_pbc(h, H.soa(pos))
    return h, typ, x, pos, L


def test_atoms_with_no_one_and_odd_numbers_of_angular_neighbours(drv):
    """A dilute gas: atoms without any angular neighbour (no trip at all), with one (a single half-filled trip) and with odd
    counts (a half-filled last trip) next to even ones."""
    h, typ, x, pos, L = _sparse_gas()
    n = len(typ)
    cnt = np.zeros(n, dtype=np.int64)
    for lo in range(0, n, 512):  # neighbours inside rc_angular = 4 A, minimum image
        d = pos[lo:lo + 512, None, :] - pos[None, :, :]
        d -= L * np.rint(d / L)
        cnt[lo:lo + 512] = ((d * d).sum(axis=2) < 16.0).sum(axis=1) - 1
    print("angular neighbour counts:", np.bincount(cnt))
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 3).any() and (cnt == 2).any(), np.bincount(cnt)
    model = drv.model(H.golden("PbTe", "nep.txt"))
    a, b = _per_call(drv, model, h, typ, x, 0), _per_call(drv, model, h, typ, x, 1)
    _same(a, b)
    assert np.abs(a["f"]).max() > 0.0
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    (r0, nb0, _), (r1, nb1, _) = (_run(drv, model, h, typ, x, mass, 300.0, t, nsteps=50, dt_fs=1.0) for t in (0, 1))
    assert nb0 == nb1
    _same(r0, r1)


def test_decomposed_run_with_inner_ring_ghosts(monkeypatch):
    """Two ranks, forward-mode ghosts: the local engines carry ghost levels, and the kernel leaves out the pair loop of inner-ring
    ghosts whose partial forces no owned atom reads (Bufs::angf).  The ranks' engines are not reachable from here: the option's
    default comes from the environment.  20 steps at 3000 K: re-decompositions inside the run."""
    import test_dist as T
    spec = T._spec("gpu", "PbTe-reps", (4, 2, 2), (2, 1, 1), "nve", 20, 3000.0, ghosts=0)
    out = []
    for trip in ("0", "1"):
        monkeypatch.setenv("NEPMI_ANGULAR_PAIR_TRIP", trip)
        out.append(T._run_ranks(2, spec))
    for ra, rb in zip(*out):
        assert int(ra["ndec"]) == int(rb["ndec"]) and int(ra["ndec"]) >= 2
        for key in ("i0", "f0", "i1", "x1", "v1", "f1", "th1"):
            assert np.array_equal(ra[key], rb[key]), (key, np.abs(ra[key] - rb[key]).max())
