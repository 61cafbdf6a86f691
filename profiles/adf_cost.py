#!/usr/bin/env python3
"""What sampling the angular distribution function inside the run loop costs: PbTe 1,024,000 atoms (the 250-atom cell 16 x 16 x 16),
NVE, 300 K, 1 fs, one engine per variant, alternating rounds in one process, for
  narrow   `compute_adf 10 180 0 4`: the first shell, about 6 members and 15 triplets per centre atom;
  wide     `compute_adf 10 180 0 8`: about 80 members and 3,000 triplets per centre atom, 3e9 triplets per sample.

  (a) nepmi_run_nve ms/step with nothing attached and with either handle attached, alternating rounds: median (min .. max); the
      difference x 10 is the cost of one sample (binning, scan, fill, triplet kernel, accumulate);
  (b) one sample alone through nepmi_adf_sample, timed with events on the engine's stream, with the number of triplets it counted;
      the RDF sample (`compute_rdf 8 200 10`) on the same input next to it;
  (c) where oracle/_ref/gpumd_ref exists: the reference's own program and gpumd-mi on the same input with and without the keyword,
      as cost per sample: (time with - time without) / samples.  For the wide range the reference's 32-bit bins overflow (2.2e9
      triplets per sample): it is timed only, its values are not compared.

Measured, not asserted.

    python profiles/adf_cost.py [--reps 16] [--steps 200] [--rounds 3] [--out profiles/adf_cost.json]
    python profiles/adf_cost.py --samples-only 6 --range wide      (under a profiler)
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
BINS, INTERVAL = 180, 10
RANGES = {"narrow": (0.0, 4.0), "wide": (0.0, 8.0)}


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), rounds=[float(x) for x in v])


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])


def keyword(which):
    return "compute_adf %d %d %g %g" % (INTERVAL, BINS, RANGES[which][0], RANGES[which][1])


def in_process(drv, torch, nep, h, typ, x, mass, args, out):
    import helpers as H
    from gpumd_amd.nep import ADF, RDF
    n = len(typ)
    vel = H.maxwell_velocities(mass, 300.0, seed=4)
    dt = 1.0 / H.TIME_UNIT
    model = drv.model(nep)
    res = out["pbte"] = dict(atoms=n, num_bins=BINS, interval=INTERVAL, steps_per_round=args.steps)

    def fresh(which):
        eng = drv.engine(model, n)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
        adf = None
        if which:
            adf = ADF(eng, RANGES[which], BINS, INTERVAL)
            eng.attach(adf)
        eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st, adf

    def run(eng, st, steps):
        eng.run_nve(h, st["t"], st["m"], dt, steps, st["x"], st["v"], st["pe"], st["f"], st["w"], thermo_every=steps)

    variants = {"nothing_attached": fresh(None), "narrow": fresh("narrow"), "wide": fresh("wide")}
    ms = {k: [] for k in variants}
    for eng, st, _ in variants.values():
        run(eng, st, args.warmup)
    for _ in range(args.rounds):
        for key, (eng, st, _) in variants.items():
            drv.sync()
            t0 = time.perf_counter()
            run(eng, st, args.steps)
            drv.sync()
            ms[key].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res["run_nve_ms_per_step"] = {k: spread(v) for k, v in ms.items()}
    base = res["run_nve_ms_per_step"]["nothing_attached"]["median"]
    print("[pbte, %d atoms] run_nve ms/step, nothing attached: %s" % (n, fmt(res["run_nve_ms_per_step"]["nothing_attached"])))
    for which in RANGES:
        r = res[which] = dict(keyword=keyword(which), form=variants[which][2].form)
        r["ms_per_sample_in_the_loop"] = spread([(a - b) * INTERVAL for a, b in zip(ms[which], ms["nothing_attached"])])
        r["added_per_step_percent"] = 100.0 * (res["run_nve_ms_per_step"][which]["median"] / base - 1.0)
        counts, ns = variants[which][2].read()
        r["samples_in_the_loop"] = ns
        r["triplets_per_sample_in_the_loop"] = float(counts.sum()) / max(ns, 1)
        print("[pbte] %s (form %d): %s ms/step -> %+.1f %% per step, %s ms per sample in the loop"
              % (keyword(which), r["form"], fmt(res["run_nve_ms_per_step"][which]), r["added_per_step_percent"], fmt(r["ms_per_sample_in_the_loop"])))

    # (b) one sample alone
    eng0, st0, _ = variants["nothing_attached"]

    def alone(handle, total):
        handle.sample(st0["x"], h, (1, 1, 1))
        t = []
        for _ in range(3 * args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            handle.sample(st0["x"], h, (1, 1, 1))
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        s = spread(t)
        s["counted_per_sample"] = float(total(handle)) / (1 + 3 * args.rounds)
        handle.close()
        return s

    for which in RANGES:
        s = res[which]["one_sample"] = alone(ADF(eng0, RANGES[which], BINS, 1), lambda a: a.read()[0].sum())
        s["triplets_per_ns"] = s["counted_per_sample"] / (s["median"] * 1e6)
        print("[pbte] one sample through nepmi_adf_sample, %s: %s ms; %.4g triplets counted, %.2f per ns"
              % (keyword(which), fmt(s), s["counted_per_sample"], s["triplets_per_ns"]))
    s = res["rdf_one_sample"] = alone(RDF(eng0, 8.0, 200, 1, typ, 2), lambda r: r.read()[0].sum())
    print("[pbte] one sample through nepmi_rdf_sample, compute_rdf 8 200 10: %s ms; %.4g pairs counted" % (fmt(s), s["counted_per_sample"]))
    for eng, st, adf in variants.values():
        if adf is not None:
            adf.close()
        eng.close()
    del variants
    torch.cuda.empty_cache()


def binaries(args, out):
    import ref_compare as R
    if not os.path.exists(R.REF):
        print("oracle/_ref/gpumd_ref is not built: the reference's cost per sample is not measured")
        out.setdefault("not_measured", []).append("reference binary (not built)")
        return
    steps = {"none": args.ref_steps, "narrow": args.ref_steps, "wide": args.ref_steps_wide}
    samples = {k: v // INTERVAL for k, v in steps.items()}
    configs = {"none": "", "narrow": keyword("narrow") + "\n", "wide": keyword("wide") + "\n"}
    res = {exe: {k: [] for k in configs} for exe in ("gpumd_ref", "gpumd_mi")}
    base = os.path.join(args.scratch, "adf_cost_runs")
    for rnd in range(args.ref_rounds):
        for key, extra in configs.items():
            for tag, exe in (("gpumd_ref", R.REF), ("gpumd_mi", R.MI)):
                d = os.path.join(base, "%s_%s" % (tag, key))
                shutil.rmtree(d, ignore_errors=True)
                os.makedirs(d)
                shutil.copy(os.path.join(R.GOLD, "PbTe", "model.xyz"), os.path.join(d, "model.xyz"))
                shutil.copy(os.path.join(R.GOLD, "PbTe", "nep.txt"), os.path.join(d, "nep.txt"))
                with open(os.path.join(d, "run.in"), "w") as f:
                    f.write("replicate %d %d %d\npotential nep.txt\nvelocity 300\nensemble nve\ntime_step 1\n%srun %d\n"
                            % (args.reps, args.reps, args.reps, extra, steps[key]))
                r, _ = R.run_binary(exe, d, 600.0)
                if r["rc"] != 0 or r["run_seconds"] is None:
                    raise SystemExit("%s failed on %s: see %s/stdout.txt" % (tag, key, d))
                res[tag][key].append(r["run_seconds"])
                print("  round %d %-9s %-6s %d steps %.3f s" % (rnd, tag, key, steps[key], r["run_seconds"]), flush=True)
    shutil.rmtree(base, ignore_errors=True)
    o = out["pbte"]["binaries"] = dict(steps=steps, samples=samples, rounds=args.ref_rounds,
                                       note="wide: the reference's int bins overflow at 2.2e9 triplets per sample; timed only, values not compared")
    for tag in res:
        q = {k: spread(v) for k, v in res[tag].items()}
        for which in RANGES:  # the run without the keyword, scaled to the steps of the run with it
            q["ms_per_sample_" + which] = spread([(a - b * steps[which] / steps["none"]) * 1e3 / samples[which]
                                                  for a, b in zip(res[tag][which], res[tag]["none"])])
        o[tag] = q
        print("[pbte] %-9s none %.3f s (%d steps), narrow %.3f s (%d steps), wide %.3f s (%d steps) -> %s / %s ms per sample"
              % (tag, q["none"]["median"], steps["none"], q["narrow"]["median"], steps["narrow"], q["wide"]["median"], steps["wide"],
                 fmt(q["ms_per_sample_narrow"]), fmt(q["ms_per_sample_wide"])))


def samples_only(drv, nep, h, typ, x, args):
    """for a profiler run: a few samples of one range through nepmi_adf_sample, nothing else"""
    from gpumd_amd.nep import ADF
    eng = drv.engine(drv.model(nep), len(typ))
    a = ADF(eng, RANGES[args.range], BINS, 1)
    d_x = drv.dev(x)
    for _ in range(args.samples_only):
        a.sample(d_x, h, (1, 1, 1))
    counts, ns = a.read()
    print("%s: %d samples, %.4g triplets per sample" % (keyword(args.range), ns, float(counts.sum()) / ns))
    a.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref-steps", type=int, default=100)
    ap.add_argument("--ref-steps-wide", type=int, default=20)
    ap.add_argument("--ref-rounds", type=int, default=3)
    ap.add_argument("--samples-only", type=int, default=0)
    ap.add_argument("--range", choices=sorted(RANGES), default="narrow")
    ap.add_argument("--no-binaries", action="store_true")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adf_cost.json"))
    args = ap.parse_args()
    import torch
    import helpers as H
    drv = H.GpuDriver()
    out = dict(rounds=args.rounds)
    h, typ, x = H.pbte_supercell((args.reps,) * 3, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    if args.samples_only:
        samples_only(drv, H.golden("PbTe", "nep.txt"), h, typ, x, args)
        return
    in_process(drv, torch, H.golden("PbTe", "nep.txt"), h, typ, x, mass, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print("written: " + args.out)

    write()
    if not args.no_binaries:
        binaries(args, out)
        write()


if __name__ == "__main__":
    main()
