"""`compute_rdf` of gpumd-mi against the reference's own program on the same GPU: oracle/_ref/gpumd_ref (see test_ref_md_parity.py)
and gpumd-mi run ref_compare's `pbte_16k` (16,000 atoms, velocities from model.xyz) for 40 steps with `compute_rdf 8 100 4`: ten
samples.  Skipped where the reference binary is not built.  Where oracle/_ref/gpumd_ref_mi is built (the reference's own RDF code on
this library's forces) it runs too and its deviations are printed beside gpumd-mi's.

The header line of rdf.out: equal as text.  Values, per printed number (`%.5f`):
    |d| <= 1e-5 + m_w x (weight of one pair in that bin and column),   m_w = 2 + ceil(8 E_w),
E_w the expected number of pairs within delta of the bin's two edges over all samples, from the reference's own g in the adjoining
bins: samples x N rho 4 pi r^2 g x 2 delta per edge (partials: N_a rho_b and the partial g).  A pair's weight: total
2 V / (N^2 dV R), a-a 2 V / (N_a^2 dV R), a-b V / (N_a N_b dV R), dV = 4 pi ((w + 0.5) dr)^2 dr, R = steps / interval.
delta = 2e-6 A, the DELTA of test_ref_md_parity_corr.py (the deviation of the two programs' positions: NOT measured for this
observable before this test ran).  The reference sums 1 / (N rho dV) per ordered pair in double with atomicAdd: its own rounding,
about 1e-16 x pairs per bin, is far below the print quantum.

The test prints the largest deviation in units of one pair's weight."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

pytestmark = pytest.mark.gpu

STEPS, RC, BINS, INTERVAL = 40, 8.0, 100, 4
DELTA = 2e-6  # A


def _block(path):
    lines = open(path).read().splitlines()
    return lines[0], np.array([[float(x) for x in r.split()] for r in lines[1:]])


def _allowance(ref_rows, n_of_type, volume):
    """-> weight of one pair [BINS, 4] (columns total, 0-0, 0-1, 1-1) and m_w [BINS, 4] from the reference's own g"""
    samples = STEPS // INTERVAL
    dr = RC / BINS
    r = (np.arange(BINS) + 0.5) * dr
    dV = 4.0 * np.pi * r * r * dr
    N = float(sum(n_of_type))
    na, nb = float(n_of_type[0]), float(n_of_type[1])
    weight = np.stack([2.0 * volume / (N * N * dV), 2.0 * volume / (na * na * dV), volume / (na * nb * dV),
                       2.0 * volume / (nb * nb * dV)], axis=1) / samples
    pairs_per_length = np.array([N * N, na * na, na * nb, nb * nb]) / volume  # N_a rho_b
    g = ref_rows[:, 1:5]
    gpad = np.concatenate([g[:1], g, g[-1:]], axis=0)
    m = np.zeros((BINS, 4))
    for w in range(BINS):
        e = 0.0
        for edge, g_edge in ((w * dr, 0.5 * (gpad[w] + gpad[w + 1])), ((w + 1) * dr, 0.5 * (gpad[w + 1] + gpad[w + 2]))):
            e = e + samples * pairs_per_length * 4.0 * np.pi * edge * edge * g_edge * 2.0 * DELTA
        m[w] = 2 + np.ceil(8.0 * e)
    return weight, m


def test_rdf_matches_reference_gpumd(tmp_path):
    import ref_compare as R
    from gpumd_amd import structures as S
    if not os.path.exists(R.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (needs /root/reference at build time)")
    assert os.path.exists(R.MI), "gpumd-mi is not built"
    exes = [("ref", R.REF), ("mi", R.MI)] + ([("ref_mi", R.REF_MI)] if os.path.exists(R.REF_MI) else [])
    R.FINE = STEPS
    try:
        out = {}
        for tag, exe in exes:
            d = str(tmp_path / tag)
            R.case_inputs("pbte_16k", d)
            run_in = os.path.join(d, "run.in")
            text = open(run_in).read()
            assert "\nrun %d" % STEPS in text
            open(run_in, "w").write(text.replace("\nrun ", "\ncompute_rdf %g %d %d\nrun " % (RC, BINS, INTERVAL)))
            res, _ = R.run_binary(exe, d, 300.0)
            assert res["rc"] == 0, open(os.path.join(d, "stdout.txt")).read()[-2000:]
            out[tag] = _block(os.path.join(d, "rdf.out"))
    finally:
        R.FINE = 0
    fr = S.read_xyz_frames(os.path.join(str(tmp_path / "ref"), "model.xyz"))[0]
    species = list(fr["species"])
    n_of_type = [species.count("Te"), species.count("Pb")]  # the potential's order
    volume = abs(np.linalg.det(fr["lattice"]))
    head, ref = out["ref"]
    assert head == "#radius total Te-Te Te-Pb Pb-Pb", head
    assert ref.shape == (BINS, 5) and ref[:, 1].max() > 1.0
    weight, m = _allowance(ref, n_of_type, volume)
    worst = {}
    for tag in [t for t, _ in exes if t != "ref"]:
        h1, rows = out[tag]
        assert h1 == head, (h1, head)
        assert np.array_equal(rows[:, 0], ref[:, 0])
        dev = np.abs(rows[:, 1:] - ref[:, 1:])
        worst[tag] = float((dev / weight).max())
        print("\n[%s vs gpumd_ref] rdf.out: largest |d| %.2e; in units of one pair's weight %.3g (allowance m_w: %d .. %d); "
              "largest (|d| - 1e-5) / (m_w weight) %.3g" % (tag, dev.max(), worst[tag], int(m.min()), int(m.max()),
                                                            float(((dev - 1e-5) / (m * weight)).max())))
    _, rows = out["mi"]
    assert (np.abs(rows[:, 1:] - ref[:, 1:]) <= 1e-5 + m * weight).all(), worst
