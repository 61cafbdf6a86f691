"""`compute_msd` and `compute_sdc` in gpumd-mi (gpumd_amd/host/run.cpp), in the manner of the reference's
tests/gpumd/msd/test_compute_msd.py: the run dumps the unwrapped positions and velocities of every step in double precision, and
msd.out / sdc.out are recomputed from the dumped frames in numpy -- MSD::process / SDC::process (ring of Nc frames, every sample
from the (Nc - 1)-th on a time origin), the normalisation by atoms x origins, the finite difference (MSD -> SDC) and the trapezoid
(VAC -> SDC) with the reference's unit conversions.  Values within rtol 1e-5 (`%g` prints six digits), header lines as text.

CPU tier: the host linked against the kernel emulator (tests/emu/gpumd-mi-emu); one GPU case with the product binary.  The
250-atom PbTe cell is a small box (the loop that steps on the caller's arrays and samples through nepmi_corr_sample); replicated
2 x 2 x 2 it runs the device-resident loop."""
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest

import helpers as H
from test_host_cli import _grouped_workdir

EMU = os.path.join(H.ROOT, "tests", "emu", "gpumd-mi-emu")
EXE = os.path.join(H.ROOT, "gpumd_amd", "bin", "gpumd-mi")
DT_FS = 2.0
HEAD = "potential NEP\nvelocity 1500 seed 7\nensemble nve\ntime_step 2\n"
DUMP = "dump_xyz 1 d.xyz unwrapped_position velocity precision double\n"


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "emu"), "all"], check=True)


def _workdir(tmp_path, run_in):
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copy(H.golden("PbTe", "model.xyz"), os.path.join(str(tmp_path), "model.xyz"))
    with open(os.path.join(str(tmp_path), "run.in"), "w") as f:
        f.write(run_in.replace("NEP", H.golden("PbTe", "nep.txt")))
    return str(tmp_path)


def _run(exe, wd, expect_error=None, args=()):
    res = subprocess.run([exe, *args], cwd=wd, capture_output=True, text=True, timeout=600)
    if expect_error is None:
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    else:
        assert res.returncode != 0 and expect_error in res.stdout + res.stderr, (expect_error, res.stdout[-1500:] + res.stderr[-500:])
    return res.stdout


def _blocks(path):
    """-> [(header lines, value rows)] of the blocks appended to an .out file"""
    out = []
    for line in open(path).read().splitlines():
        if line.startswith("# compute_"):
            out.append(([], []))
        if line.startswith("#"):
            out[-1][0].append(line)
        else:
            out[-1][1].append([float(x) for x in line.split()])
    return [(h, np.array(r)) for h, r in out]


def _cell_line(frame):
    return "# cell " + " ".join("%.10e" % x for x in frame["lattice"].reshape(-1))  # rows a, b, c = cpu_h[0], [3], [6], [1], ...


def _expected_msd(frames, interval, nc, groups):
    """groups: list of boolean masks -> rows [nc, 1 + 6 len(groups)] like msd.out"""
    u = np.array([f["unwrapped_position"] for f in frames[interval - 1::interval]])
    origins = len(u) - (nc - 1)
    assert origins >= 1
    dt_ps = DT_FS * interval / 1000.0
    rows = [[l * dt_ps] for l in range(nc)]
    for sel in groups:
        msd = np.zeros((nc, 3))
        for s in range(nc - 1, len(u)):
            for lag in range(nc):
                msd[lag] += ((u[s] - u[s - lag]) ** 2)[sel].sum(axis=0)
        msd = msd / (sel.sum() * origins) if sel.sum() > 0 else msd * 0.0
        sdc = np.zeros((nc, 3))
        sdc[1:] = (msd[1:] - msd[:-1]) * 0.5 / (DT_FS * interval) * 1.0e3  # A^2 / ps
        for l in range(nc):
            rows[l] += list(msd[l]) + list(sdc[l])
    return np.array(rows)


def _expected_sdc(frames, interval, nc, sel):
    v = np.array([f["vel"] for f in frames[interval - 1::interval]])  # A / fs
    origins = len(v) - (nc - 1)
    vac = np.zeros((nc, 3))
    for s in range(nc - 1, len(v)):
        for lag in range(nc):
            vac[lag] += (v[s] * v[s - lag])[sel].sum(axis=0)
    vac /= sel.sum() * origins
    sdc = np.zeros((nc, 3))
    for l in range(1, nc):
        sdc[l] = sdc[l - 1] + (vac[l - 1] + vac[l]) * 0.5 * (DT_FS * interval) * 1.0e3  # A^2 / ps
    dt_ps = DT_FS * interval / 1000.0
    return np.array([[l * dt_ps] + list(vac[l] * 1.0e6) + list(sdc[l]) for l in range(nc)])  # VAC in A^2 / ps^2


def _msd_header(spec, n, per_group, cell, interval, all_groups):
    cols = " msdx msdy msdz sdcx sdcy sdcz" if not all_groups else "".join(
        " msdx_%d msdy_%d msdz_%d sdcx_%d sdcy_%d sdcz_%d" % ((g,) * 6) for g in range(len(per_group)))
    return ["# compute_msd " + spec, "# format_version 1", "# num_atoms %d" % n, "# num_groups %d" % len(per_group),
            "# num_atoms_per_group " + " ".join("%d" % k for k in per_group), cell,
            "# dt_output %.10e ps" % (DT_FS * interval / 1000.0), "# columns time_ps" + cols]


def _sdc_header(spec, n, cell, interval):
    return ["# compute_sdc " + spec, "# format_version 1", "# num_atoms %d" % n, cell,
            "# dt_output %.10e ps" % (DT_FS * interval / 1000.0), "# columns time_ps vacx vacy vacz sdcx sdcy sdcz"]


def _self_consistency(exe, tmp_path, replicate, head=HEAD, extra="", expect=None):
    wd = _workdir(tmp_path, replicate + head + extra + "compute_msd 1 3\ncompute_sdc 1 3\n" + DUMP + "run 8\n")
    out = _run(exe, wd)
    assert expect is None or expect in out, out[-2000:]
    assert "Compute mean square displacement (MSD)." in out and "Compute self diffusion coefficient (SDC)." in out
    assert "    sample interval is 1." in out and "    number of correlation steps is 3." in out
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    n = frames[0]["n"]
    assert len(frames) == 8
    everyone = np.ones(n, dtype=bool)
    (mh, mv), = _blocks(os.path.join(wd, "msd.out"))
    (sh, sv), = _blocks(os.path.join(wd, "sdc.out"))
    assert mh == _msd_header("1 3", n, [n], _cell_line(frames[0]), 1, False), mh
    assert sh == _sdc_header("1 3", n, _cell_line(frames[-1]), 1), sh
    em, es = _expected_msd(frames, 1, 3, [everyone]), _expected_sdc(frames, 1, 3, everyone)
    print("\n[%s n=%d] msd.out max rel deviation %.2e, sdc.out %.2e" % (os.path.basename(exe), n, np.abs(mv[1:] / em[1:] - 1.0).max(),
                                                                       np.abs(sv[1:, 1:] / es[1:, 1:] - 1.0).max()))
    assert em[1:, 1:4].min() > 0.0
    np.testing.assert_allclose(mv, em, rtol=1e-5, atol=0.0)
    np.testing.assert_allclose(sv, es, rtol=1e-5, atol=0.0)


def test_msd_and_sdc_against_the_dumped_frames_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "replicate 2 2 2\n")


def test_small_box_run_samples_on_the_callers_arrays_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "")


def test_hand_stepped_run_samples_through_corr_sample_on_emulator(tmp_path):
    """two `potential` lines with `dump_observer average`: the run follows the mean of the potentials, every step goes through
    Force::compute and the per-call entry points (Run::run_segment's stepwise branch), and the correlators are sampled by the host
    through nepmi_corr_sample behind every step (Run::corr_sample_stepwise)"""
    _self_consistency(EMU, tmp_path, "", head=HEAD.replace("potential NEP\n", "potential NEP\npotential NEP\n"),
                      extra="dump_observer average 8 8 0 0\n", expect="use the average potential in the molecular dynamics run")


@pytest.mark.gpu
def test_msd_and_sdc_against_the_dumped_frames_on_gpu(tmp_path):
    _self_consistency(EXE, tmp_path, "replicate 3 3 3\n")


@pytest.mark.parametrize("option", ["group 0 1", "all_groups 0"])
def test_groups_on_emulator(tmp_path, option):
    """grouping method 0 of the fixture is by species (Te 0, Pb 1), method 1 has three groups"""
    body = HEAD + "compute_msd 1 3 %s\n" % option + ("compute_sdc 1 3 group 0 1\n" if option.startswith("group") else "") + DUMP + "run 8\n"
    wd, src = _grouped_workdir(tmp_path, "replicate 2 2 2\n" + body)
    _run(EMU, wd)
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    n = frames[0]["n"]
    species = np.array(frames[0]["species"])
    te, pb = species == "Te", species == "Pb"
    (mh, mv), = _blocks(os.path.join(wd, "msd.out"))
    if option.startswith("group"):
        assert mh == _msd_header("1 3 group 0 1", int(pb.sum()), [int(pb.sum())], _cell_line(frames[0]), 1, False), mh
        np.testing.assert_allclose(mv, _expected_msd(frames, 1, 3, [pb]), rtol=1e-5, atol=0.0)
        (sh, sv), = _blocks(os.path.join(wd, "sdc.out"))
        assert sh == _sdc_header("1 3 group 0 1", int(pb.sum()), _cell_line(frames[-1]), 1), sh
        np.testing.assert_allclose(sv, _expected_sdc(frames, 1, 3, pb), rtol=1e-5, atol=0.0)
    else:
        assert mh == _msd_header("1 3 all_groups 0", n, [int(te.sum()), int(pb.sum())], _cell_line(frames[0]), 1, True), mh
        assert mv.shape == (3, 13)
        em = _expected_msd(frames, 1, 3, [te, pb])
        assert np.abs(em[2, 1:4] / em[2, 7:10] - 1.0).min() > 1e-3  # the two species do move differently
        np.testing.assert_allclose(mv, em, rtol=1e-5, atol=0.0)


def test_save_every_and_two_runs_on_emulator(tmp_path):
    """save_every 4: copies at steps 4 and 8 (and a segment boundary of the run loop there); a second `run` appends its own
    block and does not inherit the keyword of the first"""
    wd = _workdir(tmp_path, HEAD + "compute_msd 1 3 save_every 4\n" + DUMP + "run 8\ncompute_msd 2 2\n" + DUMP + "run 8\nrun 4\n")
    _run(EMU, wd)
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 16
    n = frames[0]["n"]
    everyone = np.ones(n, dtype=bool)
    blocks = _blocks(os.path.join(wd, "msd.out"))
    assert len(blocks) == 2  # the third run has no compute_msd
    assert blocks[0][0][0] == "# compute_msd 1 3 save_every 4" and blocks[1][0][0] == "# compute_msd 2 2"
    np.testing.assert_allclose(blocks[0][1], _expected_msd(frames[:8], 1, 3, [everyone]), rtol=1e-5, atol=0.0)
    np.testing.assert_allclose(blocks[1][1], _expected_msd(frames[8:], 2, 2, [everyone]), rtol=1e-5, atol=0.0)
    for k in (4, 8):
        (h, v), = _blocks(os.path.join(wd, "msd_step%d.out" % k))
        assert h == blocks[0][0]
        np.testing.assert_allclose(v, _expected_msd(frames[:k], 1, 3, [everyone]), rtol=1e-5, atol=0.0)
    assert not os.path.exists(os.path.join(wd, "msd_step12.out")) and not os.path.exists(os.path.join(wd, "msd_step16.out"))


@pytest.mark.parametrize("line, message", [
    ("compute_msd 1", "compute_msd should have at least 2 parameters."),
    ("compute_sdc 1", "compute_sdc should have at least 2 parameters."),
    ("compute_msd 1 3 group 0 1 save_every 4 x", "compute_msd has too many parameters."),
    ("compute_sdc 1 3 group 0 1 x", "compute_sdc has too many parameters."),
    ("compute_msd 1.5 3", "sample interval should be an integer."),
    ("compute_msd 0 3", "sample interval should be positive."),
    ("compute_sdc -2 3", "sample interval should be positive."),
    ("compute_msd 1 x", "number of correlation steps should be an integer."),
    ("compute_sdc 1 0", "number of correlation steps should be positive."),
    ("compute_msd 1 3 every 4", "Unrecognized argument in compute_msd."),
    ("compute_sdc 1 3 all_groups 0", "Unrecognized argument in compute_sdc."),
    ("compute_msd 1 3 all_groups 0 group 0 1", "Cannot compute MSD over a single group and all groups at the same time"),
    ("compute_msd 1 3 group 2 0", "Grouping method should < number of grouping methods."),
    ("compute_msd 1 3 group 0 2", "Group ID should < number of groups."),
])
def test_input_errors_have_the_reference_messages(tmp_path, line, message):
    wd, _ = _grouped_workdir(tmp_path, HEAD + line + "\nrun 8\n")
    _run(EMU, wd, expect_error=message, args=("--check-input",))


@pytest.mark.parametrize("keyword, name", [("compute_msd", "MSD"), ("compute_sdc", "SDC")])
def test_more_correlation_time_than_steps_is_refused(tmp_path, keyword, name):
    """MSD::preprocess (msd.cu:217-219); the same refusal for compute_sdc, where the reference divides by zero time origins"""
    wd = _workdir(tmp_path, HEAD + keyword + " 2 5\nrun 8\n")
    _run(EMU, wd, expect_error=name + " correlation times sampling interval should be <= number of MD steps.")
    ok = _workdir(tmp_path / "ok", HEAD + keyword + " 2 4\nrun 8\n")
    _run(EMU, ok)


@pytest.mark.parametrize("keyword", ["compute_msd", "compute_sdc"])
def test_multi_rank_launch_refuses(tmp_path, keyword):
    wd = _workdir(tmp_path, "replicate 4 2 2\npotential NEP x\nvelocity 300 seed 7\nensemble nve\ntime_step 1\n" + keyword + " 1 2\nrun 4\n")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   NEPMI_TRANSPORT="tcp", OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([EMU], cwd=wd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode != 0 for p in procs), outs[0][-2000:]
    assert keyword + " is not available in multi-GPU runs" in outs[0], outs[0][-2000:]
