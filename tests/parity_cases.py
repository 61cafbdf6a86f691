"""Parity cases shared by the CPU tier (tests/emu host-loop emulator: kernel LOGIC) and the GPU
tier (the product library on an MI355X).  Every case drives the C ABI of include/nepmi.h and
checks against the oracle on the same seeded input.

Stated tolerances (FP32 kernels, FP64 accumulation into the caller's arrays):
  neighbour lists (Verlet, radial, angular)  : bit-exact index sets, ascending order
  wrapped positions                          : bit-exact
  total energy                               : rtol 1e-5              (reference TOLERANCES)
  forces vs FP64 oracle                      : |d| <= 1e-4 |f| + 3e-5 eV/A   (reference
                                               transform-invariance atol, conftest.py:81-82)
  forces vs FP32 oracle                      : |d| <= 1e-4 |f| + 2e-5 eV/A (summation order differs)
  per-atom virial vs FP64 oracle             : |d| <= 1e-4 |w| + 1e-4 eV
"""
import numpy as np

import helpers as H

MODELS = {
    # name: (nep.txt, structure builder, num_types or None)
    "PbTe-A": ("PbTe/nep.txt", lambda: H.pbte_supercell((2, 2, 2)), None),
    "PbTe-B": ("PbTe/nep_B.txt", lambda: H.pbte_supercell((2, 2, 2), seed=2), None),
    "PbTe-ortho": ("PbTe/nep.txt", lambda: H.rocksalt_orthogonal((4, 4, 5)), None),
    # 12 cells per direction: large enough for the engine to coarsen its cell grid towards full bricks
    "PbTe-3x3x3": ("PbTe/nep.txt", lambda: H.pbte_supercell((3, 3, 3), rattle=0.03, seed=6), None),
    "PbTe-ortho-big": ("PbTe/nep.txt", lambda: H.rocksalt_orthogonal((7, 8, 7)), None),
    "C-2022": ("C/nep.txt", lambda: H.diamond((6, 6, 7), 3.57), 1),
    "C-nep3": ("C/nep3.txt", lambda: H.diamond((6, 7, 6), 3.57, seed=10), 1),
    "UNEP-v1": ("UNEP/nep.txt", lambda: H.fcc_alloy((5, 5, 6), 3.9, 16), 16),
    # large enough for the LDS-window kernels (13 cells per direction): many-type force assembly from the neighbours' Fp rows
    "UNEP-v1-big": ("UNEP/nep.txt", lambda: H.fcc_alloy((12, 12, 12), 3.9, 16, seed=8), 16),
    "BaZrO3": ("BaZrO3/nep.txt", lambda: H.pbte_supercell((2, 2, 2), num_types=3, seed=4), 3),
    "water-model": ("water/nep.txt", lambda: H.pbte_supercell((2, 2, 2), num_types=2, seed=5), 2),
    # the other shipped potentials/nep models: 3-/4-/5-body silicon, long-range carbon (rc 7/4, 16 radial basis)
    "Si-3body": ("Si/nep_3body.txt", lambda: H.diamond((4, 4, 4), 5.43, seed=21), 1),
    "Si-4body": ("Si/nep_4body.txt", lambda: H.diamond((4, 4, 5), 5.43, seed=22), 1),
    "Si-5body": ("Si/nep_5body.txt", lambda: H.diamond((4, 5, 4), 5.43, seed=23), 1),
    "C-2024": ("C/nep_2024.txt", lambda: H.diamond((6, 6, 6), 3.57, seed=24), 1),
    # eight cells of 4 A per direction: the LDS-window kernels on the largest windows they take (5,832 atoms in one window; rc 7 A:
    # ~380 Verlet entries per atom, bricks of ~730 atoms = three passes of a workgroup)
    "C-2024-window": ("C/nep_2024.txt", lambda: H.diamond((9, 9, 9), 3.567, rattle=0.04, seed=25), 1),
}


def check_force_parity(drv, name, generic=False, check_lists=True, tiles=True, mfma=True, lanes=None, win_static=None,
                       force_form=None, f32_atol=2e-5, brick=None):
    nep_rel, build, _ = MODELS[name]
    nep = H.golden(*nep_rel.split("/"))
    h, typ, x = build()
    n = len(typ)
    if name == "C-2024-window":
        # ~380 radial neighbours per atom: the FP32 oracle and the engine each stay within 3e-5 eV/A of the FP64 forces (asserted
        # below with the suite's tolerance) and, summing in different orders, up to twice that apart
        f32_atol = max(f32_atol, 6e-5)
    orc = H.Oracle(nep)
    pe32, f32, v32, q32, fp32 = orc.compute(typ, h, x, precision=32, path=0, stages=True)
    pe64, f64, v64 = orc.compute(typ, h, x, precision=64, path=0)

    model = drv.model(nep)
    assert model.info.dim == orc.info.dim and model.info.num_types == orc.info.num_types
    eng = drv.engine(model, n)
    if generic:
        eng.set_generic(True)
    eng.set_tiles(tiles)
    if not mfma:
        eng.set_mfma(False)
    if lanes is not None:
        eng.set_win_lanes(lanes)
    if win_static is not None:
        eng.set_win_static(win_static)
    if force_form is not None:
        eng.set_force_form(force_form)
    if brick is not None:
        eng.set_brick_force(brick)
    if name == "C-2024-window" and tiles:
        eng.set_option("win_max_atoms", 6656)  # (shapes without type-pure lists -- the cover shape of this tier -- stop at 5,000 by default)
    xw, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    if not tiles:
        assert eng.stats().radial_tiles == 0
    elif name == "C-2024-window":
        assert eng.stats().radial_tiles != 0, eng.describe()  # (the case exists for the window kernels on their largest windows)
    if win_static is not None and tiles is True and lanes == 1:  # (0: the box is too small for windows at all)
        assert eng.stats().radial_tiles in (0, 3 if win_static else 2)

    assert np.array_equal(xw, H.oracle_apply_pbc(h, x)), "wrapped positions must be bit-exact"
    np.testing.assert_allclose(pe.sum(), pe64.sum(), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(pe, pe64, rtol=1e-5, atol=2e-5)
    assert np.all(np.abs(f - f64) <= 1e-4 * np.abs(f64) + 3e-5), np.abs(f - f64).max()
    assert np.all(np.abs(f - f32) <= 1e-4 * np.abs(f32) + f32_atol), np.abs(f - f32).max()
    assert np.all(np.abs(v - v64) <= 1e-4 * np.abs(v64) + 1e-4), np.abs(v - v64).max()
    # total virial (what thermo/stress uses)
    vt, vt64 = v.reshape(9, n).sum(axis=1), v64.reshape(9, n).sum(axis=1)
    np.testing.assert_allclose(vt, vt64, rtol=1e-4, atol=1e-3 * np.sqrt(n) * 1e-2)
    # Newton's third law: the forces of a periodic system sum to zero (to FP32 accumulation noise)
    assert np.abs(f.reshape(3, n).sum(axis=1)).max() < 1e-4 * np.sqrt(n)

    # stage-wise: descriptors and dU/dq
    q = drv.zeros(orc.info.dim * n, dtype=np.float32)
    fp = drv.zeros(orc.info.dim * n, dtype=np.float32)
    eng.descriptors(q, fp)
    q, fp = drv.host(q).reshape(-1, n), drv.host(fp).reshape(-1, n)
    np.testing.assert_allclose(q, q32, rtol=2e-5, atol=2e-5 * np.abs(q32).max())
    np.testing.assert_allclose(fp, fp32, rtol=2e-4, atol=2e-4 * np.abs(fp32).max())

    if check_lists:
        L = orc.lists(typ, h, x, path=0)
        for which, key in ((2, "skin"), (0, "radial"), (1, "angular")):
            onn, onl = L[key]
            mx, nn, nl = H.engine_lists(drv, eng, n, which, ld=int(onn.max()) + 2)
            assert mx == onn.max()
            H.assert_lists_equal(nn, nl, onn, onl)
        st = eng.stats(True)
        assert st.max_nn_radial == L["radial"][0].max() and st.max_nn_angular == L["angular"][0].max()
        assert abs(st.mean_nn_radial - L["radial"][0].mean()) < 1e-9
    return eng


def check_translation_and_wrap(drv):
    """Lattice-vector shifts and a rigid translation change nothing but FP32 rounding
    (tests_pytest/test_invariances.py)."""
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((2, 2, 2), seed=21)
    n = len(typ)
    model = drv.model(nep)
    eng = drv.engine(model, n)
    _, pe0, f0, v0 = H.engine_force(drv, eng, h, typ, x)
    H3 = np.asarray(h).reshape(3, 3)
    shift = np.zeros(3 * n)
    rng = np.random.default_rng(3)
    k = rng.integers(-1, 2, (n, 3))  # move every atom by its own lattice vector combination
    d = k @ H3.T
    x2 = x + d.T.reshape(-1)
    eng2 = drv.engine(model, n)
    xw, pe1, f1, v1 = H.engine_force(drv, eng2, h, typ, x2)
    np.testing.assert_allclose(pe1.sum(), pe0.sum(), rtol=1e-6)
    assert np.abs(f1 - f0).max() < 3e-5
    # rigid translation
    t = np.array([0.37, -1.91, 2.5])
    x3 = x + np.repeat(t, n)
    eng3 = drv.engine(model, n)
    _, pe2, f2, _ = H.engine_force(drv, eng3, h, typ, x3)
    np.testing.assert_allclose(pe2.sum(), pe0.sum(), rtol=1e-6)
    assert np.abs(f2 - f0).max() < 3e-5


def check_rotation_permutation_and_finite_differences(drv, name="PbTe-A"):
    """tests_pytest/test_invariances.py:47-97 and test_force_energy_consistency.py:47-61 through the C ABI, with the
    reference suite's tolerances (conftest.py:81-93): energy rtol 1e-4 + 1e-5 eV, force rtol 1e-4 + 3e-5 eV/A,
    finite differences (1e-2 A central) rtol 1e-2 + 4e-3 eV/A."""
    nepf, build, _ = MODELS[name]
    nep = H.golden(*nepf.split("/"))
    h, typ, x = build()
    n = len(typ)
    model = drv.model(nep)

    def evaluate(hh, tt, xx):
        eng = drv.engine(model, n)
        _, pe, f, _ = H.engine_force(drv, eng, hh, tt, xx)
        return pe.sum(), f.reshape(3, n)

    e0, f0 = evaluate(h, typ, x)
    # the suite's 3e-5 eV/A floor was set on fixtures whose forces stay below ~1 eV/A; the rattled carbon cell reaches
    # 5.5 eV/A, and FP32 rounding of a re-oriented sum scales with that: floor = max(3e-5, 1e-5 |f|_max)
    atol = max(3e-5, 1e-5 * np.abs(f0).max())
    # rotation by 37 degrees about (0.3, 0.5, 0.811...) of cell and coordinates: E the same, F co-rotates
    axis = np.array([0.3, 0.5, 0.8113883008])
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    th = np.deg2rad(37.0)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    H3 = np.asarray(h).reshape(3, 3)  # columns a, b, c
    e1, f1 = evaluate((R @ H3).reshape(9), typ, (R @ x.reshape(3, n)).reshape(-1))
    assert abs(e1 - e0) <= 1e-4 * abs(e0) + 1e-5
    np.testing.assert_allclose(f1, R @ f0, rtol=1e-4, atol=atol)
    # cyclic relabelling inside every species: E the same, F follows the atoms
    perm = np.arange(n)
    for t in np.unique(typ):
        idx = np.nonzero(typ == t)[0]
        if len(idx) > 1:
            perm[idx] = np.roll(idx, 1)
    assert not np.array_equal(perm, np.arange(n))
    e2, f2 = evaluate(h, typ[perm], x.reshape(3, n)[:, perm].reshape(-1))
    assert abs(e2 - e0) <= 1e-4 * abs(e0) + 1e-5
    np.testing.assert_allclose(f2, f0[:, perm], rtol=1e-4, atol=atol)
    # analytic force = -dE/dx by central differences, first and last atom, all directions
    for atom in (0, n - 1):
        for d in range(3):
            xp, xm = x.copy(), x.copy()
            xp[d * n + atom] += 1e-2
            xm[d * n + atom] -= 1e-2
            num = -(evaluate(h, typ, xp)[0] - evaluate(h, typ, xm)[0]) / 2e-2
            assert abs(num - f0[d, atom]) <= 1e-2 * abs(f0[d, atom]) + 4e-3, (atom, d, num, f0[d, atom])


def check_average_of_two_potentials(drv):
    """Force::compute in the "average" mode (force.cu:533-562): two NEP models accumulate into the same arrays
    (potential_compute adds), then gpu_average_properties divides by their number."""
    h, typ, x = H.pbte_supercell((2, 2, 2), seed=91)
    n = len(typ)
    files = [H.golden("PbTe", "nep.txt"), H.golden("PbTe", "nep_B.txt")]
    engines = [drv.engine(drv.model(f), n) for f in files]
    d_t, d_x = drv.dev(typ), drv.dev(x)
    d_pe, d_f, d_w = drv.dev(np.full(n, 7.0)), drv.dev(np.full(3 * n, 7.0)), drv.dev(np.full(9 * n, 7.0))
    engines[0].apply_pbc(h, d_x)
    engines[0].zero_properties(d_pe, d_f, d_w)
    for e in engines:
        e.compute(h, d_t, d_x, d_pe, d_f, d_w)  # Potential::compute: adds
    engines[0].average_properties(2, d_pe, d_f, d_w)
    xw = drv.host(d_x)
    ref = [H.Oracle(f).compute(typ, h, xw, precision=64, path=0) for f in files]
    pe, f, w = [(ref[0][k] + ref[1][k]) / 2 for k in range(3)]
    np.testing.assert_allclose(drv.host(d_pe).sum(), pe.sum(), rtol=1e-5)
    np.testing.assert_allclose(drv.host(d_f), f, rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(drv.host(d_w), w, rtol=1e-4, atol=1e-4)
    # the division itself is exact IEEE: averaging one potential with denominator 1 changes nothing
    before = drv.host(d_f)
    engines[0].average_properties(1, d_pe, d_f, d_w)
    assert np.array_equal(drv.host(d_f), before)


def check_nve_against_oracle(drv, nsteps=20, reps=(2, 2, 2)):
    """Run::perform_a_run (nve): trajectory, thermo and rebuild policy vs the oracle's loop."""
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell(reps, rattle=0.02, seed=31)
    n = len(typ)
    orc = H.Oracle(nep)
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 6000.0, seed=5)  # hot: forces a list rebuild within the run
    dt = 2.0 / H.TIME_UNIT
    # initial forces
    pe0, f0, v0 = orc.compute(typ, h, x, precision=32, path=0)
    ref = orc.run_nve(typ, h, x, vel, mass, dt, nsteps, precision=32)

    model = drv.model(nep)
    eng = drv.engine(model, n)
    d_t, d_m = drv.dev(typ), drv.dev(mass)
    d_x, d_v = drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)  # Run: initial force before the loop
    th = eng.run_nve(h, d_t, d_m, dt, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    xs, vs = drv.host(d_x), drv.host(d_v)
    assert th.shape == (nsteps, 8)
    # positions are FP64 state driven by FP32 forces: agreement degrades slowly with steps
    H3 = np.asarray(h).reshape(3, 3)
    dx = (xs - ref["pos"]).reshape(3, n)
    frac = np.linalg.solve(H3, dx)
    frac -= np.rint(frac)
    assert np.abs(H3 @ frac).max() < 1e-6
    assert np.abs(vs - ref["vel"]).max() < 1e-6
    np.testing.assert_allclose(th[:, 0], ref["thermo"][:, 0], rtol=1e-6)   # temperature
    np.testing.assert_allclose(th[:, 1], ref["thermo"][:, 1], rtol=1e-6)   # potential energy
    np.testing.assert_allclose(th[:, 2:], ref["thermo"][:, 2:], rtol=1e-4, atol=1e-6)
    st = eng.stats()
    assert st.num_rebuild == ref["rebuilds"], (st.num_rebuild, ref["rebuilds"])
    assert st.num_rebuild >= 2
    # energy conservation over the short run (test_md_conservation.py: drift < 2e-3 dt^2 N)
    ke = 1.5 * n * H.K_B * th[:, 0]
    etot = ke + th[:, 1]
    assert np.abs(etot - etot[0]).max() < 2e-3 * (2.0 ** 2) * n


def check_unwrapped_positions(drv, nsteps=24):
    """Atom::unwrapped_position (integrate.cu:312-372): the fused loops add every un-wrapped drift to the
    caller's array; bit-identical to new - old taken around the stand-alone first half-step."""
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.02, seed=77)
    n = len(typ)
    orc = H.Oracle(nep)
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 3000.0, seed=8)
    dt = 2.0 / H.TIME_UNIT
    model = drv.model(nep)

    # fused run with the unwrapped array registered (records every 5 steps: seam and plain halves both run)
    eng = drv.engine(model, n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    d_u = drv.dev(x.copy())
    eng.set_tiles(2)  # both engines on one force-assembly variant: the comparison below is bit for bit
    eng.set_unwrapped(d_u)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    eng.run_nve(h, d_t, d_m, dt, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    unw, xs = drv.host(d_u), drv.host(d_x)
    eng.set_unwrapped(None)

    # the same trajectory through the stand-alone calls, unwrapped kept on the host
    eng2 = drv.engine(model, n)
    eng2.set_tiles(2)
    e_x, e_v = drv.dev(x), drv.dev(vel)
    e_pe, e_f, e_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng2.force_compute(h, d_t, e_x, e_pe, e_f, e_w)
    ref = x.copy()
    for _ in range(nsteps):
        old = drv.host(e_x)
        eng2.vv_step1(dt, d_m, e_f, e_x, e_v)
        ref += drv.host(e_x) - old
        eng2.force_compute(h, d_t, e_x, e_pe, e_f, e_w)
        eng2.vv_step2(dt, d_m, e_f, e_v)
    assert np.array_equal(xs, drv.host(e_x))
    assert np.array_equal(unw, ref)
    # unwrapped - wrapped is a lattice vector, and some atoms did leave the cell
    H3 = np.asarray(h).reshape(3, 3)
    frac = np.linalg.solve(H3, (unw - xs).reshape(3, n))
    assert np.abs(frac - np.rint(frac)).max() < 1e-9
    assert np.abs(np.rint(frac)).max() >= 1


def check_streaming_ops(drv):
    """apply_pbc, velocity-Verlet halves and find_thermo alone, against the oracle (FP64)."""
    h, typ, x = H.pbte_supercell((2, 2, 2), seed=41)
    n = len(typ)
    rng = np.random.default_rng(2)
    mass = np.where(typ == 0, 127.6, 207.2)
    vel = rng.normal(0, 0.01, 3 * n)
    f = rng.normal(0, 1.0, 3 * n)
    pe = rng.normal(-3, 0.1, n)
    w = rng.normal(0, 1.0, 9 * n)
    xs = x + rng.normal(0, 3.0, 3 * n)  # some atoms outside the cell
    model = drv.model(H.golden("PbTe", "nep.txt"))
    eng = drv.engine(model, n)
    d_x = drv.dev(xs)
    eng.apply_pbc(h, d_x)
    assert np.array_equal(drv.host(d_x), H.oracle_apply_pbc(h, xs))
    # vv
    L = H.oracle_lib()
    dt = 1.0 / H.TIME_UNIT
    xo, vo = x.copy(), vel.copy()
    L.nepo_velocity_verlet(1, n, dt, H._p(mass, H._dp), H._p(f, H._dp), H._p(xo, H._dp), H._p(vo, H._dp))
    d_x, d_v, d_f, d_m = drv.dev(x), drv.dev(vel), drv.dev(f), drv.dev(mass)
    eng.vv_step1(dt, d_m, d_f, d_x, d_v)
    assert np.array_equal(drv.host(d_x), xo) and np.array_equal(drv.host(d_v), vo)
    L.nepo_velocity_verlet(0, n, dt, H._p(mass, H._dp), H._p(f, H._dp), H._p(xo, H._dp), H._p(vo, H._dp))
    eng.vv_step2(dt, d_m, d_f, d_v)
    assert np.array_equal(drv.host(d_v), vo)
    # thermo
    vol = abs(np.linalg.det(np.asarray(h).reshape(3, 3)))
    tho = H.oracle_thermo(vol, mass, pe, vo, w)
    d_th = drv.zeros(8)
    eng.find_thermo(vol, d_m, drv.dev(pe), d_v, drv.dev(w), d_th)
    np.testing.assert_allclose(drv.host(d_th), tho, rtol=1e-12, atol=1e-12)


def check_small_box(drv):
    """NEP::compute's small-box branch (a periodic thickness <= 2.5 (rc + 1)): the reference's own
    CUDA known answer for PbTe-250 (examples/gpumd_static/dump.xyz) and the BaZrO3-40 golden
    regression of tests_pytest, plus the oracle's small-box lists (repeated periodic images)."""
    # --- PbTe 250 atoms: config 1 of BASELINE.json, now on the device ---
    nep = H.golden("PbTe", "nep.txt")
    fr = H.read_xyz_frames(H.golden("PbTe", "model.xyz"))[0]
    orc = H.Oracle(nep)
    typ = H.types_from_species(fr["species"], orc.symbols)
    x = H.soa(fr["pos"])
    n = fr["n"]
    model = drv.model(nep)
    eng = drv.engine(model, n)
    xw, pe, f, v = H.engine_force(drv, eng, fr["h"], typ, x)
    ref = H.read_xyz_frames(H.golden("PbTe", "dump.xyz"))[0]
    np.testing.assert_allclose(pe.sum(), ref["energy"], rtol=1e-5)
    assert np.abs(f.reshape(3, n).T - ref["forces"]).max() < 2e-5        # check_force.m:9
    vt = v.reshape(9, n).sum(axis=1)
    got = np.array([vt[0], vt[3], vt[4], vt[6], vt[1], vt[5], vt[7], vt[8], vt[2]])
    np.testing.assert_allclose(got, ref["virial"], rtol=1e-4, atol=2e-3)
    xo = H.oracle_apply_pbc(fr["h"], x)
    pe32, f32, v32 = orc.compute(typ, fr["h"], xo, precision=32, path=-1)
    assert np.all(np.abs(f - f32) <= 1e-4 * np.abs(f32) + 2e-5)
    assert np.all(np.abs(v - v32) <= 1e-4 * np.abs(v32) + 1e-4)
    L = orc.lists(typ, fr["h"], xo)
    assert L["path"] == 1
    for which, key in ((0, "radial"), (1, "angular")):
        onn, onl = L[key]
        mx, nn, nl = H.engine_lists(drv, eng, n, which, ld=int(onn.max()) + 2)
        assert mx == onn.max()
        H.assert_lists_equal(nn, nl, onn, onl)
    # --- BaZrO3 40 atoms (8 A cell, rc 8 A: many images of the same atom) ---
    nep = H.golden("BaZrO3", "nep.txt")
    fr = H.read_xyz_frames(H.golden("BaZrO3", "BaZrO3-nat40-rattled.xyz"))[0]
    model = drv.model(nep)
    typ = H.types_from_species(fr["species"], model.symbols)
    g = np.load(H.golden("BaZrO3", "bulk_bazro3.npz"))
    eng = drv.engine(model, fr["n"])
    _, pe, f, v = H.engine_force(drv, eng, fr["h"], typ, H.soa(fr["pos"]))
    np.testing.assert_allclose(pe.sum(), float(g["energy"]), rtol=1e-5)
    np.testing.assert_allclose(f.reshape(3, -1).T, g["forces"], rtol=1e-4, atol=3e-5)
    vol = abs(np.linalg.det(fr["lattice"]))
    vt = v.reshape(9, -1).sum(axis=1)
    stress = -np.array([vt[0], vt[1], vt[2], vt[5], vt[4], vt[3]]) / vol
    np.testing.assert_allclose(stress, g["stress"], rtol=1e-4, atol=1e-6)
    # --- a short NVE run in the small box against the oracle loop ---
    nep = H.golden("PbTe", "nep.txt")
    fr = H.read_xyz_frames(H.golden("PbTe", "model.xyz"))[0]
    orc = H.Oracle(nep)
    typ = H.types_from_species(fr["species"], orc.symbols)
    n = fr["n"]
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 600.0, seed=8)
    x = H.oracle_apply_pbc(fr["h"], H.soa(fr["pos"]))
    ref = orc.run_nve(typ, fr["h"], x, vel, mass, 1.0 / H.TIME_UNIT, 5, precision=32)
    eng = drv.engine(drv.model(nep), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(fr["h"], d_t, d_x, d_pe, d_f, d_w)
    th = eng.run_nve(fr["h"], d_t, d_m, 1.0 / H.TIME_UNIT, 5, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    assert np.abs(drv.host(d_v) - ref["vel"]).max() < 1e-6
    np.testing.assert_allclose(th[:, :2], ref["thermo"][:, :2], rtol=1e-6)


def check_nvt_berendsen(drv, nsteps=30):
    """`ensemble nvt_ber 300 600 20`: VV + find_thermo + gpu_berendsen_temperature
    (ensemble_ber.cu:70-86, 195-235) against the same loop built from oracle pieces."""
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.01, seed=51)
    n = len(typ)
    orc = H.Oracle(nep)
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 300.0, seed=6)
    dt = 1.0 / H.TIME_UNIT
    t1, t2, tc = 300.0, 600.0, 20.0
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt)
    th_ref, _ = loop.run("ber", nsteps, t1, t2, tc)
    vo = loop.v
    eng = drv.engine(drv.model(nep), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    th = eng.run_nvt_ber(h, d_t, d_m, dt, nsteps, t1, t2, tc, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    np.testing.assert_allclose(th[:, 0], th_ref[:, 0], rtol=1e-6)
    np.testing.assert_allclose(th[:, 1], th_ref[:, 1], rtol=1e-6)
    assert np.abs(drv.host(d_v) - vo).max() < 1e-6
    assert th[-1, 0] > th[0, 0]  # the thermostat heats the crystal towards the 600 K target


def check_nvt_nhc(drv, nsteps=30):
    """`ensemble nvt_nhc 300 500 50`: integrate_nvt_nhc_1/2 (ensemble_nhc.cu:166-232) with the chain
    advanced on the device, against the same loop built from oracle pieces (host chain, nepo_nhc)."""
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.01, seed=52)
    n = len(typ)
    orc = H.Oracle(nep)
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 300.0, seed=7)
    dt = 1.0 / H.TIME_UNIT
    t1, t2, tc = 300.0, 500.0, 50.0
    vol = abs(np.linalg.det(np.asarray(h).reshape(3, 3)))
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt)
    th_ref, _ = loop.run("nhc", nsteps, t1, t2, tc)
    vo, st, fac = loop.v, loop.chain, loop.factors
    assert min(fac) < 1.0 < max(fac) or max(abs(np.array(fac) - 1.0)) > 1e-6  # the chain really acts

    eng = drv.engine(drv.model(nep), n)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    th = eng.run_nvt_nhc(h, d_t, d_m, dt, nsteps, t1, t2, tc, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    np.testing.assert_allclose(th[:, 0], th_ref[:, 0], rtol=1e-6)
    np.testing.assert_allclose(th[:, 1], th_ref[:, 1], rtol=1e-6)
    assert np.abs(drv.host(d_v) - vo).max() < 1e-6

    # the step-level entries give the same trajectory as the one-call loop
    d_x, d_v = drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng2 = drv.engine(drv.model(nep), n)
    eng2.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    d_st, d_th = drv.zeros(eng2.NHC_STATE_SIZE), drv.zeros(8)
    eng2.nhc_init(t1, tc, dt, d_st)
    for step in range(nsteps):
        target = t1 + (t2 - t1) * (step / nsteps)
        eng2.find_thermo(vol, d_m, d_pe, d_v, d_w, d_th)
        eng2.nhc_half_step(target, dt, d_th, d_st, d_v)
        eng2.vv_step1(dt, d_m, d_f, d_x, d_v)
        eng2.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
        eng2.vv_step2(dt, d_m, d_f, d_v)
        eng2.find_thermo(vol, d_m, d_pe, d_v, d_w, d_th)
        eng2.nhc_half_step(target, dt, d_th, d_st, d_v)
    # the two engines may settle on different (equivalent) kernel variants: agreement to f32 summation order
    np.testing.assert_allclose(drv.host(d_th)[0], th[-1, 0], rtol=1e-7)
    chain = drv.host(d_st)
    np.testing.assert_allclose(chain[:12], st, rtol=5e-5, atol=1e-9)  # f32 force noise feeds the chain


def check_angular_recompute(drv):
    """The angular force kernel's two sources of the s sums (stored by the descriptor kernel / rebuilt
    from the compact records) are the same arithmetic in the same order; on the device the two inlined
    copies may contract multiply-adds differently, so agreement is to f32 rounding, not bitwise."""
    for name in ("PbTe-A", "C-2022", "UNEP-v1"):
        nep_rel, build, _ = MODELS[name]
        model = drv.model(H.golden(*nep_rel.split("/")))
        h, typ, x = build()
        out = []
        for mode in (0, 1):
            eng = drv.engine(model, len(typ))
            eng.set_angular_recompute(mode)
            out.append(H.engine_force(drv, eng, h, typ, x))
        for a, b in zip(out[0][1:], out[1][1:]):
            assert np.abs(a - b).max() <= 2e-6 * max(1.0, np.abs(a).max()), name


def check_nvt_bdp(drv, nsteps=30, seed=20240924):
    """`ensemble nvt_bdp 300 500 50` with a fixed seed: integrate_nvt_bdp_2 (ensemble_bdp.cu:71-104) against the
    same loop built from oracle pieces; the oracle restates MT19937 and libstdc++'s canonical-double draw, so the
    stochastic factors must agree draw for draw, not just statistically."""
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((2, 2, 2), rattle=0.01, seed=53)
    n = len(typ)
    orc = H.Oracle(nep)
    mass = np.array([H.MASS[orc.symbols[t]] for t in typ])
    vel = H.maxwell_velocities(mass, 300.0, seed=8)
    dt = 1.0 / H.TIME_UNIT
    t1, t2, tc = 300.0, 500.0, 50.0
    loop = H.OracleLoop(orc, typ, h, x, vel, mass, dt, bdp_seed=seed)
    th_ref, _ = loop.run("bdp", nsteps, t1, t2, tc)
    vo, fac = loop.v, np.array(loop.factors)
    assert np.abs(fac - 1.0).max() > 1e-4 and fac.min() < 1.0 < fac.max()  # noise of both signs

    eng = drv.engine(drv.model(nep), n)
    eng.bdp_seed(seed)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    th = eng.run_nvt_bdp(h, d_t, d_m, dt, nsteps, t1, t2, tc, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    np.testing.assert_allclose(th[:, 0], th_ref[:, 0], rtol=1e-6)
    np.testing.assert_allclose(th[:, 1], th_ref[:, 1], rtol=1e-6)
    assert np.abs(drv.host(d_v) - vo).max() < 1e-6
    # another seed gives another trajectory
    eng2 = drv.engine(drv.model(nep), n)
    eng2.bdp_seed(seed + 1)
    d_x, d_v = drv.dev(x), drv.dev(vel)
    eng2.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    th2 = eng2.run_nvt_bdp(h, d_t, d_m, dt, nsteps, t1, t2, tc, d_x, d_v, d_pe, d_f, d_w, thermo_every=1)
    assert np.abs(th2[:, 0] - th[:, 0]).max() > 1e-3


def check_error_paths(drv):
    import pytest
    from gpumd_amd import NepmiError
    model = drv.model(H.golden("PbTe", "nep.txt"))
    # wrong atom count
    h, typ, x = H.pbte_supercell((2, 2, 2))
    eng = drv.engine(model, len(typ) - 1)
    with pytest.raises(NepmiError):
        H.engine_force(drv, eng, h, typ, x)
    # a blown-up simulation (NaN / huge coordinates) is reported, it neither hangs nor faults
    for bad in (np.nan, np.inf):
        eng = drv.engine(model, len(typ))
        xb = np.array(x)
        xb[7] = bad
        with pytest.raises(NepmiError, match="non-finite|capacity"):
            n = len(typ)
            d_t, d_x = drv.dev(typ), drv.dev(xb)
            d_pe, d_f, d_v = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
            eng.compute(h, d_t, d_x, d_pe, d_f, d_v)
            eng.stats()
    # unsupported / malformed model files
    with pytest.raises(NepmiError):
        drv.model(H.golden("PbTe", "model.xyz"))
    with pytest.raises(NepmiError):
        drv.model(H.golden("PbTe", "does_not_exist.txt"))


def check_boundary_conditions(drv):
    """Free and mixed boundaries (Box::pbc_x/y/z = 0, box.cuh:84-129: no minimum image and no wrap
    along a free direction; neighbor.cuh:76-110: cell index clamped) and degenerate inputs: an atom
    with no neighbours at all, and an engine used below its capacity."""
    nep = H.golden("PbTe", "nep.txt")
    orc = H.Oracle(nep)
    model = drv.model(nep)
    h0, typ, x0 = H.pbte_supercell((2, 2, 2), seed=11)
    n = len(typ)
    for pbc in ((0, 0, 0), (1, 1, 0), (0, 1, 1), (1, 0, 0)):
        # vacuum along the free directions: the cell keeps its shape, atoms sit in the middle
        h = np.array(h0, dtype=np.float64).reshape(-1)[:9].copy().reshape(3, 3)
        x = np.array(x0).reshape(3, n).copy()
        for d in range(3):
            if not pbc[d]:
                h[:, d] *= 1.6
        frac = np.linalg.solve(np.array(h0).reshape(-1)[:9].reshape(3, 3), x)
        for d in range(3):
            if not pbc[d]:
                frac[d] = (frac[d] + 0.3) / 1.6
        x = (h @ frac).reshape(-1)
        h9 = h.reshape(-1)
        pe64, f64, v64 = orc.compute(typ, h9, H.oracle_apply_pbc(h9, x, pbc), pbc=pbc, precision=64, path=0)
        eng = drv.engine(model, n, pbc=pbc)
        xw, pe, f, v = H.engine_force(drv, eng, h9, typ, x)
        assert np.array_equal(xw, H.oracle_apply_pbc(h9, x, pbc)), pbc
        np.testing.assert_allclose(pe, pe64, rtol=1e-5, atol=2e-5)
        assert np.all(np.abs(f - f64) <= 1e-4 * np.abs(f64) + 3e-5), (pbc, np.abs(f - f64).max())
        assert np.all(np.abs(v - v64) <= 1e-4 * np.abs(v64) + 1e-4), pbc
        L = orc.lists(typ, h9, xw, pbc=pbc, path=0)
        for which, key in ((0, "radial"), (1, "angular")):
            onn, onl = L[key]
            mx, nn, nl = H.engine_lists(drv, eng, n, which, ld=int(onn.max()) + 2)
            H.assert_lists_equal(nn, nl, onn, onl)
        # surface atoms really lost neighbours
        assert L["radial"][0].min() < L["radial"][0].max()

    # isolated atoms: three atoms 40 A apart in a 120 A box -> no neighbours, E_i = ANN(q = 0)
    h9 = np.diag([120.0, 120.0, 120.0]).reshape(-1)
    typ3 = np.array([0, 1, 0], dtype=np.int32)
    x3 = H.soa(np.array([[10.0, 10.0, 10.0], [50.0, 50.0, 50.0], [90.0, 90.0, 90.0]]))
    pe64, f64, v64 = orc.compute(typ3, h9, x3, precision=64, path=0)
    eng = drv.engine(model, 3)
    _, pe, f, v = H.engine_force(drv, eng, h9, typ3, x3)
    np.testing.assert_allclose(pe, pe64, rtol=1e-5, atol=1e-6)
    assert np.abs(f).max() == 0.0 and np.abs(v).max() == 0.0 and np.abs(f64).max() == 0.0
    assert pe[0] == pe[2] and pe[0] != pe[1]

    # capacity > n: one engine serves a smaller system than it was created for
    eng = drv.engine(model, 2 * n)
    h9 = np.array(h0, dtype=np.float64).reshape(-1)[:9]
    pe64, f64, _ = orc.compute(typ, h9, x0, precision=64, path=0)
    _, pe, f, _ = H.engine_force(drv, eng, h9, typ, np.array(x0))
    np.testing.assert_allclose(pe, pe64, rtol=1e-5, atol=2e-5)
    assert np.all(np.abs(f - f64) <= 1e-4 * np.abs(f64) + 3e-5)


# ---------------------------------------------------------------------------------------------------------------------
# Full-size parity: the sizes the metric is quoted on (BASELINE config 3) and >= 250 k atoms of the many-type and carbon
# models.  The window kernels take their list decisions in a fixed-point frame and retake them exactly only inside a
# band that grows with the box length (engine_impl.h: WinGeom::band), so the three lists are compared with the oracle's
# entry for entry and the forces / virials of EVERY atom with the oracle's where the box is largest.
# The oracle's sweeps are shared among the host's cores (OpenMP; bit-identical to the serial sweep).
# ---------------------------------------------------------------------------------------------------------------------
FULL_SIZE = {
    # name: (nep.txt, builder, atoms)
    "PbTe-1M-triclinic": ("PbTe/nep.txt", lambda: H.pbte_supercell((16, 16, 16), rattle=0.02, seed=42), 1024000),
    "PbTe-1M-orthogonal": ("PbTe/nep.txt", lambda: H.rocksalt_orthogonal((40, 40, 80), rattle=0.01, seed=42), 1024000),
    "UNEP-256k": ("UNEP/nep.txt", lambda: H.fcc_alloy((40, 40, 40), 3.9, 16, rattle=0.01, seed=42), 256000),
    "C-262k": ("C/nep.txt", lambda: H.diamond((32, 32, 32), 3.57, seed=42), 262144),
    # CPU-tier stand-ins: the same box LENGTH along a (371.7 A: the band is as wide as in the 1 M-atom box), fewer atoms
    "PbTe-bar-64k": ("PbTe/nep.txt", lambda: H.pbte_supercell((16, 4, 4), rattle=0.02, seed=42), 64000),
    "PbTe-ortho-bar": ("PbTe/nep.txt", lambda: H.rocksalt_orthogonal((80, 8, 8), rattle=0.01, seed=42), 40960),
}


def check_full_size_parity(drv, name):
    import time
    nep_rel, build, natoms = FULL_SIZE[name]
    nep = H.golden(*nep_rel.split("/"))
    t0 = time.time()
    h, typ, x = build()
    n = len(typ)
    assert n == natoms
    orc = H.Oracle(nep)
    L = orc.lists(typ, h, x, path=0)
    pe32, f32, v32 = orc.compute(typ, h, x, precision=32, path=0)
    pe64, f64, v64 = orc.compute(typ, h, x, precision=64, path=0)
    t_oracle = time.time() - t0
    t0 = time.time()
    eng = drv.engine(drv.model(nep), n)
    xw, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    assert eng.stats().radial_tiles >= 1, "the LDS-window kernels are what this case is about"
    assert np.array_equal(xw, H.oracle_apply_pbc(h, x)), "wrapped positions must be bit-exact"
    # every entry of the three lists
    for which, key in ((2, "skin"), (0, "radial"), (1, "angular")):
        onn, onl = L[key]
        mx, nn, nl = H.engine_lists(drv, eng, n, which, ld=int(onn.max()) + 2)
        assert mx == onn.max()
        assert np.array_equal(nn, onn), "%s list: %d atoms with a different count" % (key, int((nn != onn).sum()))
        ld = onl.shape[0]
        for s0 in range(0, ld, 16):  # in slabs of 16 slots (memory)
            s1 = min(s0 + 16, ld)
            mask = (np.arange(s0, s1)[:, None] < onn[None, :])
            a, b = nl[s0:s1][mask], onl[s0:s1][mask]
            assert np.array_equal(a, b), "%s list: %d entries differ" % (key, int((a != b).sum()))
        del nn, nl
    # every atom's energy, force and virial
    np.testing.assert_allclose(pe.sum(), pe64.sum(), rtol=1e-5)
    np.testing.assert_allclose(pe, pe64, rtol=1e-5, atol=2e-5)
    d64 = np.abs(f - f64) - 1e-4 * np.abs(f64)
    assert d64.max() <= 3e-5, "forces vs FP64 oracle: worst excess %.3e" % d64.max()
    # The FP32 oracle forms r12 like the reference's kernels: float(double difference) + float minimum image.  For a
    # pair that crosses a periodic face of a ~370 A box that carries ~3e-5 A of rounding; the
    # engine's fixed-point geometry does not, so the comparison with the FP32 oracle is held to the FP32 oracle's own
    # distance from the FP64 one plus the usual summation-order term.
    own = np.abs(f32 - f64)
    d32 = np.abs(f - f32) - 1e-4 * np.abs(f32) - own
    assert d32.max() <= 2e-5, "forces vs FP32 oracle: worst excess %.3e" % d32.max()
    dv = np.abs(v - v64) - 1e-4 * np.abs(v64)
    assert dv.max() <= 1e-4, "virials vs FP64 oracle: worst excess %.3e" % dv.max()
    vt, vt64 = v.reshape(9, n).sum(axis=1), v64.reshape(9, n).sum(axis=1)
    np.testing.assert_allclose(vt, vt64, rtol=1e-4, atol=1e-5 * np.sqrt(n))
    assert np.abs(f.reshape(3, n).sum(axis=1)).max() < 1e-4 * np.sqrt(n)
    st = eng.stats(True)
    assert st.max_nn_radial == L["radial"][0].max() and st.max_nn_angular == L["angular"][0].max()
    df_gather = np.abs(f - f64).max()
    # the same positions through the scatter form of the force assembly -- the form the run loops (and the bench line) take at
    # this size; per-call evaluations use the gather form unless asked
    eng.set_force_form(1)
    _, pe_s, f_s, v_s = H.engine_force(drv, eng, h, typ, x)
    scattered = "lds_scatter_of_own_halves" in eng.describe()
    if isinstance(drv, H.GpuDriver) and "lanes_per_atom=1" in eng.describe():  # (few bricks: several lanes per atom, gather form)
        assert scattered, eng.describe()
    assert np.array_equal(pe_s, pe)  # energies: the same kernels
    ds = np.abs(f_s - f64) - 1e-4 * np.abs(f64)
    assert ds.max() <= 3e-5, "scatter form: forces vs FP64 oracle, worst excess %.3e" % ds.max()
    dvs = np.abs(v_s - v64) - 1e-4 * np.abs(v64)
    assert dvs.max() <= 1e-4, "scatter form: virials vs FP64 oracle, worst excess %.3e" % dvs.max()
    if scattered and not name.startswith("UNEP"):
        # +g and -g are the same integer: the total force vanishes to the FP64 rounding of the fold (UNEP adds ZBL in floating point)
        assert np.abs(f_s.reshape(3, n).sum(axis=1)).max() < 1e-6
    if scattered:
        # ... and with the per-step lists in the form the run loops write them since round 6 -- the radial list as wave-synchronous
        # words, the angular records as padded rows rebuilt from the LDS window (nep_window.h: SyncFifo) -- which a per-call
        # evaluation takes when only the total virial is owed (virial mode 1 = the run loops' rule): the same pairs, the same
        # per-pair arithmetic in the same order into integer sums, so forces and energies are the scatter form's bit for bit
        eng.set_virial_mode(1)
        _, pe_y, f_y, v_y = H.engine_force(drv, eng, h, typ, x)
        assert "wave_synchronous_words" in eng.describe() and "lds_scatter_of_own_halves" in eng.describe(), eng.describe()
        assert np.array_equal(f_y, f_s) and np.array_equal(pe_y, pe_s)
        np.testing.assert_allclose(v_y.reshape(9, n).sum(axis=1), vt64, rtol=1e-4, atol=1e-5 * np.sqrt(n))
        eng.set_virial_mode(0)
        _, pe_z, f_z, v_z = H.engine_force(drv, eng, h, typ, x)  # back to the compact lists and the reference's virial attribution
        assert np.array_equal(f_z, f_s) and np.array_equal(v_z, v_s)
    print("\n[full-size parity] %s: %d atoms, oracle %.1f s, engine + comparison %.1f s, max|dF| vs FP64 %.2e (gather) %.2e (scatter), "
          "vs FP32 %.2e" % (name, n, t_oracle, time.time() - t0, df_gather, np.abs(f_s - f64).max(), np.abs(f - f32).max()))
    return eng
