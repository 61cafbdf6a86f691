"""`compute_orientorder` of gpumd-mi against the reference's own program on the same GPU: oracle/_ref/gpumd_ref (see
test_ref_md_parity.py) and gpumd-mi run ref_compare's `pbte_16k` (16,000 atoms, velocities from model.xyz) for 40 steps, once with
`compute_orientorder 4 cutoff 3.95 2 4 6 1 1 1` and once with `compute_orientorder 4 nnn 6 2 4 6 0 1 1`: ten blocks each; both
programs dump double-precision frames at the sample steps.  Skipped where the reference binary is not built.

(a) The reference's orientorder.out against the numpy restatement (test_orient_kernels.restate) on the REFERENCE's own frames: all
columns within the print quantum (`%f`: 5e-7, plus 1e-9).  Left out are atoms with a neighbour within a relative 4e-7 of the cutoff
(the reference's list is cut in float), and with `average` the atoms one of whose members is such; asserted: at most 1e-3 of the
atoms.  This pins the restatement, and with it every other test of this observable, on the reference's program.  The restatement
walks the pairs of 16,000 atoms, seconds a frame, so it is made for the first, the middle and the last block.
(b) gpumd-mi's file against the reference's: `step` and header lines equal as text in every block.  In the restated blocks the q_l
columns agree within the bound of test_run_orient.py -- sqrt(l (l + 1)) delta mean_j(1 / d_ij), its mean over the atom and its members
with `average`, delta = 2e-6 A (the DELTA of the other parity tests: the deviation of the two programs' positions) -- plus the print
quantum of both files, 1e-6.  One rule leaves atoms out of (a) and (b): a neighbour within max(delta, 4e-7 rc) of the cutoff, in mode
nnn also the k-th and (k+1)-th distances closer than twice that.  For w_l and what_l no tolerance is fixed in
advance (their agreement on identical positions is what (a) and test_host_orient.py assert): the largest deviation is printed."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import helpers as H  # noqa: E402
import test_host_orient as HO  # noqa: E402
import test_orient_kernels as OK  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, INTERVAL = 40, 4
DELTA = 2e-6  # A
DEGREES = [4, 6]
FORMS = {"cutoff": ("compute_orientorder 4 cutoff 3.95 2 4 6 1 1 1", ("cutoff", 3.95, True)),
         "nnn": ("compute_orientorder 4 nnn 6 2 4 6 0 1 1", ("nnn", 6, False))}


@pytest.mark.parametrize("form", list(FORMS))
def test_orientorder_matches_reference_gpumd(tmp_path, form):
    import ref_compare as R
    if not os.path.exists(R.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (needs the reference's sources at build time)")
    assert os.path.exists(R.MI), "gpumd-mi is not built"
    line, (mode, value, average) = FORMS[form]
    R.FINE = STEPS
    try:
        out, frames = {}, {}
        for tag, exe in (("ref", R.REF), ("mi", R.MI)):
            d = str(tmp_path / tag)
            R.case_inputs("pbte_16k", d)
            run_in = os.path.join(d, "run.in")
            text = open(run_in).read()
            assert "\nrun %d" % STEPS in text
            open(run_in, "w").write(text.replace("\nrun ", "\n%s\ndump_xyz %d d.xyz precision double\nrun " % (line, INTERVAL)))
            res, _ = R.run_binary(exe, d, 300.0)
            assert res["rc"] == 0, open(os.path.join(d, "stdout.txt")).read()[-2000:]
            out[tag] = HO.blocks_of(os.path.join(d, "orientorder.out"))
            frames[tag] = H.read_xyz_frames(os.path.join(d, "d.xyz"))
    finally:
        R.FINE = 0
    nblocks = STEPS // INTERVAL
    assert len(out["ref"]) == len(out["mi"]) == len(frames["ref"]) == nblocks
    header = HO.header_of(DEGREES, True, True)
    for k in range(nblocks):
        for tag in ("ref", "mi"):
            assert out[tag][k][0] == "step = %d" % ((k + 1) * INTERVAL) and out[tag][k][1] == header, out[tag][k][:2]
            assert out[tag][k][2].shape == (16000, 6)
    worst_w = worst_q = worst_a = 0.0
    for k in (0, nblocks // 2, nblocks - 1):
        fr = frames["ref"][k]
        pos = np.ascontiguousarray(fr["pos"].T)
        rc = value if mode == "cutoff" else 6.0
        band = max(DELTA, 4e-7 * rc)  # one rule for (a) and (b): a neighbour within 4e-7 relative of the cutoff, or within delta of it
        pre = OK.bonds(pos, fr["h"], fr["pbc"], mode, value, delta=band)
        ref = OK.restate(pos, fr["h"], fr["pbc"], mode, value, DEGREES, average, True, True, delta=band, pre=pre)
        assert ref["amb"].mean() <= 1e-3, ref["amb"].sum()
        ok = ~ref["amb"]
        # (a)
        assert np.isfinite(out["ref"][k][2]).all() and ref["nn"].min() > 0
        dev = np.abs(out["ref"][k][2] - ref["cols"])[ok]
        worst_a = max(worst_a, float(dev.max()))
        assert (dev <= HO.QUANTUM).all(), (k, float(dev.max()), np.argwhere(dev > HO.QUANTUM)[:5])
        # (b): the two programs' positions differ by delta
        b = DELTA * ref["minv"]
        if average:
            b = (b + np.bincount(ref["ci"], weights=b[ref["cj"]], minlength=len(b))) / (ref["nn"] + 1.0)
        bound = b[:, None] * np.array([math.sqrt(l * (l + 1.0)) for l in DEGREES])[None, :] + 1e-6
        d = np.abs(out["mi"][k][2] - out["ref"][k][2])
        worst_q = max(worst_q, float(d[ok, :2].max()))
        worst_w = max(worst_w, float(d[ok, 2:].max()))
        assert (d[ok, :2] <= bound[ok]).all(), (k, float(d[ok, :2].max()))
    print("\n[%s] gpumd_ref against the restatement on its own frames: largest |d column| %.2e (quantum 5e-7)" % (form, worst_a))
    print("[%s] gpumd-mi against gpumd_ref: largest |d ql| %.2e, largest |d wl|, |d wlhat| %.2e (print quantum of both 1e-6)"
          % (form, worst_q, worst_w))
