"""`compute_msd` / `compute_sdc` of gpumd-mi against the reference's own program on the same GPU: oracle/_ref/gpumd_ref (see
test_ref_md_parity.py) and gpumd-mi run ref_compare's `carbon_nve` (64,000 atoms, velocities from model.xyz) for 60 steps with
`compute_msd 2 10` and `compute_sdc 2 10`: 30 samples, 21 time origins.  Skipped where the reference binary is not built.

Header lines of msd.out and sdc.out: equal as text.  Values, per printed number (`%g`: six digits, so each of the two printed
numbers carries up to 5e-6 of itself in print quantisation, q below):
  MSD:  |d| <= 2 sqrt(MSD) delta + delta^2 + q,  delta = 2e-6 A the deviation of the two programs' positions (NOT measured: the
        per-coordinate tolerance of the run-loop tests, twice, for a difference of two positions);
  the SDC columns of msd.out, (MSD_l - MSD_(l-1)) / (2 dt): the two MSD bounds over 2 dt, + q;
  VAC:  |d| <= 2e-6 VAC_0 + q  (the T / K tolerance of test_ref_md_parity.CASES["carbon_nve"], 2e-6 relative on a product of two
        velocities; sum|v v'| <= sum v^2 = VAC_0 x atoms x origins by Cauchy-Schwarz);
  SDC of sdc.out, the trapezoid over the VAC: |d| <= 2e-6 VAC_0 x (l dt) + q.
Where oracle/_ref/gpumd_ref_mi is built (the reference's own MSD and SDC code on this library's forces) it runs too and its
deviations from the reference are printed beside gpumd-mi's: that pair shows what the force path alone contributes.

Measured on an MI355X: gpumd-mi against gpumd_ref differs by at most one unit of the last printed digit -- MSD 1e-9 A^2 (1.6e-6
relative), VAC 1e-5 of VAC_0 = 11.49, both SDC columns 1e-7 -- which is 1.4 % of the msd.out bound and 19 % of the sdc.out bound: the
delta above held.  gpumd_ref_mi against gpumd_ref: the same figures."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

pytestmark = pytest.mark.gpu

STEPS, INTERVAL, NC = 60, 2, 10
DELTA = 2e-6  # A
Q = 5e-6      # print quantisation of one `%g` number, relative


def _blocks(path):
    head, rows = [], []
    for line in open(path).read().splitlines():
        (head if line.startswith("#") else rows).append(line)
    return head, np.array([[float(x) for x in r.split()] for r in rows])


def _bounds(msd_ref, sdc_ref):
    """-> bound arrays for the 7 columns of msd.out and of sdc.out, from the reference's own numbers"""
    dt_ps = msd_ref[1, 0] - msd_ref[0, 0]
    m = msd_ref[:, 1:4]
    bm = 2.0 * np.sqrt(m) * DELTA + DELTA ** 2
    bs = np.zeros_like(bm)
    bs[1:] = (bm[1:] + bm[:-1]) * 0.5 / dt_ps
    b_msd = np.concatenate([np.zeros((NC, 1)), bm, bs], axis=1)
    vac0 = sdc_ref[0:1, 1:4]
    lag = np.arange(NC)[:, None]
    b_sdc = np.concatenate([np.zeros((NC, 1)), 2e-6 * vac0 * np.ones((NC, 1)), 2e-6 * vac0 * lag * dt_ps], axis=1)
    return b_msd, b_sdc


def test_msd_and_sdc_match_reference_gpumd(tmp_path):
    import ref_compare as R
    from test_ref_md_parity import CASES
    if not os.path.exists(R.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (needs /root/reference at build time)")
    assert os.path.exists(R.MI), "gpumd-mi is not built"
    assert CASES["carbon_nve"][0] == 2e-6
    exes = [("ref", R.REF), ("mi", R.MI)] + ([("ref_mi", R.REF_MI)] if os.path.exists(R.REF_MI) else [])
    R.FINE = STEPS
    try:
        out = {}
        for tag, exe in exes:
            d = str(tmp_path / tag)
            R.case_inputs("carbon_nve", d)
            run_in = os.path.join(d, "run.in")
            text = open(run_in).read()
            assert "\nrun %d" % STEPS in text
            open(run_in, "w").write(text.replace("\nrun ", "\ncompute_msd %d %d\ncompute_sdc %d %d\nrun " % (INTERVAL, NC, INTERVAL, NC)))
            res, _ = R.run_binary(exe, d, 300.0)
            assert res["rc"] == 0, open(os.path.join(d, "stdout.txt")).read()[-2000:]
            out[tag] = (_blocks(os.path.join(d, "msd.out")), _blocks(os.path.join(d, "sdc.out")))
    finally:
        R.FINE = 0
    (mh, mr), (sh, sr) = out["ref"]
    assert mr.shape == (NC, 7) and sr.shape == (NC, 7)
    b_msd, b_sdc = _bounds(mr, sr)
    worst = {}
    for tag in [t for t, _ in exes if t != "ref"]:
        (h1, m1), (h2, s1) = out[tag]
        assert h1 == mh, (h1, mh)
        assert h2 == sh, (h2, sh)
        dm, ds = np.abs(m1 - mr), np.abs(s1 - sr)
        qm, qs = Q * (np.abs(m1) + np.abs(mr)), Q * (np.abs(s1) + np.abs(sr))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[tag] = (np.nanmax(np.where(b_msd + qm > 0, dm / (b_msd + qm), 0.0)), np.nanmax(np.where(b_sdc + qs > 0, ds / (b_sdc + qs), 0.0)))
        print("\n[%s vs gpumd_ref] msd.out: max |d| msd %.3e A^2 (rel %.2e), sdc %.3e; sdc.out: max |d| vac %.3e (of VAC_0 %.3e), sdc %.3e;"
              " largest |d| / bound: msd.out %.3g, sdc.out %.3g"
              % (tag, dm[:, 1:4].max(), (dm[1:, 1:4] / mr[1:, 1:4]).max(), dm[:, 4:].max(), ds[:, 1:4].max(), sr[0, 1:4].min(),
                 ds[:, 4:].max(), worst[tag][0], worst[tag][1]))
    (_, m1), (_, s1) = out["mi"]
    assert (np.abs(m1 - mr) <= b_msd + Q * (np.abs(m1) + np.abs(mr))).all(), worst
    assert (np.abs(s1 - sr) <= b_sdc + Q * (np.abs(s1) + np.abs(sr))).all(), worst
