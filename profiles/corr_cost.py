#!/usr/bin/env python3
"""What sampling a correlation function inside the run loop costs: PbTe, 1,024,000 atoms (the 250-atom cell 16 x 16 x 16), NVE,
300 K, 1 fs, on one engine per variant, alternating rounds in one process:

  (a) nepmi_run_nve ms/step with nothing attached, with an MSD correlator (`compute_msd 10 100`) and with a VAC correlator
      (`compute_sdc 10 100`) attached; the rounds start after 1000 warm-up steps, so every sample is a time origin and the
      difference x 10 is the cost of one sample (gather + correlation over 100 lags);
  (b) one sample through nepmi_corr_sample on a full ring, timed with events on the engine's stream, against the kernel's
      compulsory bytes (Nc + 1) n 24 (2.4 GB here: 0.30 ms at the 8 TB/s peak);
  (c) where oracle/_ref/gpumd_ref exists: the reference's own program and gpumd-mi on the same input with and without the two
      keywords, 2000 steps (200 samples, 101 of them time origins), as cost per time origin: (time with - time without) / 101.

Alternating runs, three rounds, the spread is printed; measured, not asserted.

    python profiles/corr_cost.py [--reps 16] [--steps 500] [--rounds 3] [--out profiles/corr_cost.json]
"""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
INTERVAL, NC = 10, 100


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), rounds=[float(x) for x in v])


def binaries(args, out):
    import ref_compare as R
    if not os.path.exists(R.REF):
        print("oracle/_ref/gpumd_ref is not built: the reference's cost per sample is not measured")
        return
    steps = args.ref_steps
    origins = steps // INTERVAL - (NC - 1)
    configs = {"none": "", "msd": "compute_msd %d %d\n" % (INTERVAL, NC), "sdc": "compute_sdc %d %d\n" % (INTERVAL, NC)}
    res = {exe: {k: [] for k in configs} for exe in ("gpumd_ref", "gpumd_mi")}
    base = os.path.join(args.scratch, "corr_cost_runs")
    for rnd in range(args.rounds):
        for key, extra in configs.items():
            for tag, exe in (("gpumd_ref", R.REF), ("gpumd_mi", R.MI)):
                d = os.path.join(base, "%s_%s" % (tag, key))
                shutil.rmtree(d, ignore_errors=True)
                os.makedirs(d)
                shutil.copy(os.path.join(R.GOLD, "PbTe", "model.xyz"), os.path.join(d, "model.xyz"))
                shutil.copy(os.path.join(R.GOLD, "PbTe", "nep.txt"), os.path.join(d, "nep.txt"))
                with open(os.path.join(d, "run.in"), "w") as f:
                    f.write("replicate %d %d %d\npotential nep.txt\nvelocity 300\nensemble nve\ntime_step 1\n%srun %d\n"
                            % (args.reps, args.reps, args.reps, extra, steps))
                r, _ = R.run_binary(exe, d, 900.0)
                if r["rc"] != 0 or r["run_seconds"] is None:
                    raise SystemExit("%s failed on %s: see %s/stdout.txt" % (tag, key, d))
                res[tag][key].append(r["run_seconds"])
                print("  round %d %-9s %-4s %.3f s" % (rnd, tag, key, r["run_seconds"]), flush=True)
    shutil.rmtree(base, ignore_errors=True)
    out["binaries"] = dict(steps=steps, time_origins=origins)
    for tag in res:
        o = {k: spread(v) for k, v in res[tag].items()}
        for k in ("msd", "sdc"):
            per = [(a - b) * 1e3 / origins for a, b in zip(res[tag][k], res[tag]["none"])]
            o[k + "_ms_per_time_origin"] = spread(per)
        out["binaries"][tag] = o
        print("%-9s run of %d steps: none %.3f s, compute_msd %.3f s, compute_sdc %.3f s -> ms per time origin: msd %.3f (%.3f .. %.3f), "
              "sdc %.3f (%.3f .. %.3f)" % (tag, steps, o["none"]["median"], o["msd"]["median"], o["sdc"]["median"],
                                          o["msd_ms_per_time_origin"]["median"], o["msd_ms_per_time_origin"]["min"],
                                          o["msd_ms_per_time_origin"]["max"], o["sdc_ms_per_time_origin"]["median"],
                                          o["sdc_ms_per_time_origin"]["min"], o["sdc_ms_per_time_origin"]["max"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref-steps", type=int, default=2000)
    ap.add_argument("--no-binaries", action="store_true")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_cost.json"))
    args = ap.parse_args()
    import torch
    import helpers as H
    from gpumd_amd.nep import Correlator
    drv = H.GpuDriver()
    nep = H.golden("PbTe", "nep.txt")
    h, typ, x = H.pbte_supercell((args.reps,) * 3, rattle=0.03, seed=17)
    n = len(typ)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    vel = H.maxwell_velocities(mass, 300.0, seed=4)
    dt = 1.0 / H.TIME_UNIT
    model = drv.model(nep)
    out = dict(atoms=n, interval=INTERVAL, num_corr=NC, steps_per_round=args.steps, rounds=args.rounds)

    def fresh(quantity):
        eng = drv.engine(model, n)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n),
                  u=drv.dev(x.copy()))
        corr = None
        if quantity:
            eng.set_unwrapped(st["u"])
            corr = Correlator(eng, quantity, INTERVAL, NC)
            eng.attach(corr)
        eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st, corr

    def run(eng, st, steps):
        eng.run_nve(h, st["t"], st["m"], dt, steps, st["x"], st["v"], st["pe"], st["f"], st["w"], thermo_every=steps)

    variants = {"nothing_attached": fresh(None), "compute_msd_10_100": fresh("msd"), "compute_sdc_10_100": fresh("vac")}
    ms = {k: [] for k in variants}
    for name, (eng, st, corr) in variants.items():  # warm-up: the rings fill, from here on every sample is a time origin
        run(eng, st, INTERVAL * NC)
    for rnd in range(args.rounds):
        for name, (eng, st, corr) in variants.items():
            drv.sync()
            t0 = time.perf_counter()
            run(eng, st, args.steps)
            drv.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    out["run_nve_ms_per_step"] = {k: spread(v) for k, v in ms.items()}
    for name, (eng, st, corr) in variants.items():
        s = out["run_nve_ms_per_step"][name]
        extra = ""
        if corr is not None:
            sums, origins, samples = corr.read()
            per = [(a - b) * INTERVAL for a, b in zip(ms[name], ms["nothing_attached"])]
            s["ms_per_sample"] = spread(per)
            s["samples"], s["time_origins"] = samples, origins
            extra = "; per sample %.3f ms (%.3f .. %.3f); %d samples, %d time origins" % (
                s["ms_per_sample"]["median"], s["ms_per_sample"]["min"], s["ms_per_sample"]["max"], samples, origins)
        print("%-20s %8.4f ms/step (rounds: %s)%s" % (name, s["median"], " ".join("%.4f" % v for v in ms[name]), extra))
    out["describe"] = variants["nothing_attached"][0].describe()

    # (b) one sample on a full ring
    eng, st, _ = variants["nothing_attached"]
    compulsory = (NC + 1) * n * 24
    out["one_sample"] = dict(compulsory_bytes=compulsory)
    for quantity, q in (("msd", st["x"]), ("vac", st["v"])):
        c = Correlator(eng, quantity, 1, NC)
        for _ in range(NC + 2):
            c.sample(q)
        t = []
        for _ in range(3 * args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c.sample(q)
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        c.close()
        s = spread(t)
        s["TB_per_s"] = compulsory / (s["median"] * 1e-3) / 1e12
        out["one_sample"][quantity] = s
        print("one %s sample (gather + %d lags + reduction): %.3f ms (%.3f .. %.3f) = %.2f TB/s of the %.2f GB it must read"
              % (quantity, NC, s["median"], s["min"], s["max"], s["TB_per_s"], compulsory / 1e9))
    for eng, st, corr in variants.values():
        if corr is not None:
            corr.close()
        eng.close()
    del variants
    torch.cuda.empty_cache()

    if not args.no_binaries:
        binaries(args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("written: " + args.out)


if __name__ == "__main__":
    main()
