"""`compute_orientorder` in gpumd-mi (gpumd_amd/host/run.cpp): the run dumps its frames with `dump_xyz ... precision double` at the
sample steps and every block of orientorder.out -- `step = <1-based step>`, the header line `ql4 ql6 wl4 ... wlhat6`, N rows of `%f`
-- is recomputed from them by the numpy restatement (test_orient_kernels.restate).  The dumped positions are the sampled ones to the
last bit, so ALL columns agree within the `%f` quantum, 5e-7, plus 1e-9; an atom is left out only if a neighbour's d2 lies within a
relative 1e-9 of rc^2 (or its k-th and (k+1)-th within 1e-9), asserted to happen to no atom.

CPU tier: the host linked against the kernel emulator (tests/emu/gpumd-mi-emu), the 250-atom PbTe cell replicated 2 x 2 x 2 (the
resident loop) and unreplicated (19 A thick: the stepwise small-box path); one GPU case with the product binary on 3 x 3 x 3.
Input errors through --check-input, with OrientOrder::parse's messages and its oddities: with no token after the degrees it stops
with "Number of paramaters exceeds ...", one token after wlhat is accepted and ignored."""
import os
import socket
import subprocess

import numpy as np
import pytest

import helpers as H
import test_host_rdf as HR
import test_orient_kernels as OK

EMU, EXE, HEAD = HR.EMU, HR.EXE, HR.HEAD
QUANTUM = 5e-7 + 1e-9
CUTOFF = ("compute_orientorder 5 cutoff 3.95 2 4 6 1 1 1", ("cutoff", 3.95, [4, 6], True, True, True))
NNN = ("compute_orientorder 5 nnn 6 2 4 6 0 1 1", ("nnn", 6, [4, 6], False, True, True))
DUMP = "\ndump_xyz 5 d.xyz precision double\n"


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "emu"), "all"], check=True)


def blocks_of(path):
    """-> [(step line, header line, values [N, ncol])]"""
    out, lines = [], open(path).read().splitlines()
    k = 0
    while k < len(lines):
        assert lines[k].startswith("step = "), lines[k]
        step, header = lines[k], lines[k + 1]
        k += 2
        rows = []
        while k < len(lines) and not lines[k].startswith("step = "):
            rows.append([float(x) for x in lines[k].split()])
            k += 1
        out.append((step, header, np.array(rows)))
    return out


def header_of(degrees, wl, wlhat):
    names = ["ql%d" % l for l in degrees] + (["wl%d" % l for l in degrees] if wl else []) + (["wlhat%d" % l for l in degrees] if wlhat else [])
    return " ".join(names)


def check_blocks(tag, blocks, frames, spec, steps):
    mode, value, degrees, average, wl, wlhat = spec
    assert len(blocks) == len(frames) == len(steps)
    for (step, header, values), fr, t in zip(blocks, frames, steps):
        assert step == "step = %d" % t and header == header_of(degrees, wl, wlhat), (step, header)
        ref = OK.restate(np.ascontiguousarray(fr["pos"].T), fr["h"], fr["pbc"], mode, value, degrees, average, wl, wlhat)
        assert not ref["amb"].any()
        assert values.shape == ref["cols"].shape
        dev = np.abs(values - ref["cols"])
        print("\n[%s %s] largest deviation of a column %.2e (quantum 5e-7), mean nn %.2f, largest ql %.3f"
              % (tag, step, dev.max(), ref["nn"].mean(), ref["ql"].max()))
        assert ref["nn"].mean() > 4 and ref["ql"].max() > 0.3
        assert (dev <= QUANTUM).all(), np.argwhere(dev > QUANTUM)[:5]


def _self_consistency(exe, tmp_path, replicate):
    for sub, (line, spec) in (("c", CUTOFF), ("n", NNN)):
        wd = HR._workdir(tmp_path / sub, replicate + HEAD + line + DUMP + "run 10\n")
        out = HR._run(exe, wd)
        expected = ["Compute Steinhardt bond-orientational order parameters.", "    every 5 steps, ", "    with 2 degrees: 4 6,"]
        if spec[0] == "cutoff":
            expected += ["    with 3.950000 angstrom cutoff,", "    average is true, wl is true and wlhat is true."]
        else:
            expected += ["    with 6 nearest neighbor atoms,", "    average is false, wl is true and wlhat is true."]
        for text in expected:
            assert text in out, (text, out[-2000:])
        frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
        assert len(frames) == 2
        check_blocks("%s %s" % (os.path.basename(exe), sub), blocks_of(os.path.join(wd, "orientorder.out")), frames, spec, (5, 10))


def test_against_the_dumped_frames_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "replicate 2 2 2\n")


def test_the_stepwise_small_box_path_on_emulator(tmp_path):
    _self_consistency(EMU, tmp_path, "")


@pytest.mark.gpu
def test_against_the_dumped_frames_on_gpu(tmp_path):
    _self_consistency(EXE, tmp_path, "replicate 3 3 3\n")


@pytest.mark.gpu
def test_the_stepwise_small_box_path_on_gpu(tmp_path):
    _self_consistency(EXE, tmp_path, "")


def test_two_runs_append_and_the_keyword_does_not_propagate_on_emulator(tmp_path):
    """a second `run` has a handle of its own and appends its blocks; the third has no compute_orientorder.  12 steps at interval 5:
    two blocks.  One degree: the singular in the printed line; the surplus token after wlhat is ignored"""
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + CUTOFF[0] + DUMP + "run 10\n"
                     + "compute_orientorder 5 nnn 6 1 6 0 0 1 surplus" + DUMP + "run 12\nrun 3\n")
    out = HR._run(EMU, wd)
    assert "    with 1 degree: 6," in out and "    average is false, wl is false and wlhat is true." in out
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 4
    blocks = blocks_of(os.path.join(wd, "orientorder.out"))
    assert len(blocks) == 4
    check_blocks("first run", blocks[:2], frames[:2], CUTOFF[1], (5, 10))
    check_blocks("second run", blocks[2:], frames[2:], ("nnn", 6, [6], False, False, True), (5, 10))


T0 = "compute_orientorder 5 cutoff 4 "


@pytest.mark.parametrize("line, message", [
    ("compute_orientorder 5 cutoff 4 1", "compute_orientorder should have at least 5 parameters."),
    ("compute_orientorder x cutoff 4 1 4 0", "interval step per sample should be an integer."),
    ("compute_orientorder 0 cutoff 4 1 4 0", "interval step per sample should be positive."),
    ("compute_orientorder 5 cutoff x 1 4 0", "cutoff should be an positive float."),
    ("compute_orientorder 5 cutoff 0 1 4 0", "cutoff should be an positive float."),
    ("compute_orientorder 5 cutoff -1 1 4 0", "cutoff should be an positive float."),
    ("compute_orientorder 5 nnn 1.5 1 4 0", "nnn should be an positive integer."),
    ("compute_orientorder 5 nnn 0 1 4 0", "nnn should be an positive integer."),
    ("compute_orientorder 5 shell 4 1 4 0", "mode_type should be cutoff or nnn."),
    (T0 + "x 4 0", "ndegrees should be an positive integer."),
    (T0 + "0 4 0", "ndegrees should be an positive integer."),
    (T0 + "3 4 6", "Must include 3 degrees."),
    (T0 + "2 4 x 0", "Degree 2 should be an positive integer."),
    (T0 + "2 -4 6 0", "Degree 1 should be an positive integer."),
    (T0 + "2 4 6", "Number of paramaters exceeds 11."),  # no token after the degrees: the reference's message for it
    (T0 + "2 4 6 1 1 1 0 0", "Number of paramaters exceeds 11."),
    (T0 + "2 4 6 x", "average should be 1 or 0."),
    (T0 + "2 4 6 1 x", "wl should be 1 or 0."),
    (T0 + "2 4 6 1 1 x", "wlhat should be 1 or 0."),
    # ours
    (T0 + "1 13 0", "compute_orientorder takes degrees up to 12."),
    (T0 + "9 1 2 3 4 5 6 7 8 9 0", "compute_orientorder takes at most 8 degrees."),
    (T0 + "1 4 0\n" + T0 + "1 6 0", "compute_orientorder can be used once in a run."),
])
def test_input_errors_have_the_reference_messages(tmp_path, line, message):
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + line + "\nrun 10\n")
    HR._run(EMU, wd, expect_error=message, args=("--check-input",))


@pytest.mark.parametrize("tail, flags", [("0", "average is false, wl is false and wlhat is false."),
                                         ("2 0", "average is true, wl is false and wlhat is false."),
                                         ("0 1 1", "average is false, wl is true and wlhat is true."),
                                         ("1 1 1 ignored", "average is true, wl is true and wlhat is true.")])
def test_accepted_forms(tmp_path, tail, flags):
    """one to three flags; a fourth token is accepted and ignored, as the reference does"""
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + "compute_orientorder 5 nnn 12 8 2 4 6 8 10 12 6 3 " + tail + "\nrun 10\n")
    out = HR._run(EMU, wd, args=("--check-input",))
    assert "    with 8 degrees: 2 4 6 8 10 12 6 3," in out and "    with 12 nearest neighbor atoms," in out and flags in out


def test_an_overflowed_handle_ends_the_run_with_the_capacity(tmp_path):
    """rc = 14 A in PbTe (0.03 atoms / A^3): about 340 neighbours, above the capacity"""
    wd = HR._workdir(tmp_path, "replicate 2 2 2\n" + HEAD + "compute_orientorder 1 cutoff 14 1 4 0\nrun 2\n")
    HR._run(EMU, wd, expect_error="compute_orientorder: an atom has more than 320 neighbours")
    path = os.path.join(wd, "orientorder.out")
    assert not os.path.exists(path) or os.path.getsize(path) == 0


def test_the_box_is_too_thin_for_the_search_radius(tmp_path):
    """19 A thick: rc = 8 A asks for 20 A, at the first sample"""
    wd = HR._workdir(tmp_path, HEAD + "compute_orientorder 1 cutoff 8 1 4 0\nrun 2\n")
    HR._run(EMU, wd, expect_error="thickness < 2.5 cutoffs")


def test_multi_rank_launch_refuses(tmp_path):
    wd = HR._workdir(tmp_path, "replicate 4 2 2\npotential NEP x\nvelocity 300 seed 7\nensemble nve\ntime_step 1\n"
                     "compute_orientorder 2 cutoff 4 1 4 0\nrun 4\n")
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
    assert "compute_orientorder is not available in multi-GPU runs" in outs[0], outs[0][-2000:]
