#!/usr/bin/env python3
"""What sampling the Steinhardt order parameters inside the run loop costs: PbTe 1,024,000 atoms (the 250-atom cell 16 x 16 x 16),
NVE, 300 K, 1 fs, one engine per variant, alternating rounds in one process, for
  cutoff       `compute_orientorder 10 cutoff 4.0 2 4 6 0`: about 6 members per centre atom, q4 and q6;
  cutoff_all   `compute_orientorder 10 cutoff 4.0 2 4 6 1 1 1`: the same with the neighbour average, w_l and what_l;
  nnn          `compute_orientorder 10 nnn 12 2 4 6 0`: the search radius of 6 A holds about 26 atoms, the 12 nearest are kept.

  (a) nepmi_run_nve ms/step with nothing attached and with each handle attached, alternating rounds: median (min .. max); the
      difference x 10 is the cost of one sample (binning, scan, fill, q_lm kernel, average pass, columns);
  (b) one sample alone through nepmi_orient_sample, timed with events on the engine's stream;
  (c) where oracle/_ref/gpumd_ref exists: the reference's own program and gpumd-mi on the same input with and without the keyword,
      as cost per sample: (time with - time without) / samples.  Both programs also write their N rows of text per sample there.

Measured, not asserted.

    python profiles/orient_cost.py [--reps 16] [--steps 200] [--rounds 3] [--out profiles/orient_cost.json]
    python profiles/orient_cost.py --samples-only 6 --variant cutoff_all      (under a profiler)
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
INTERVAL, DEGREES = 10, [4, 6]
#            mode, value, average, wl, wlhat
VARIANTS = {"cutoff": ("cutoff", 4.0, 0, 0, 0), "cutoff_all": ("cutoff", 4.0, 1, 1, 1), "nnn": ("nnn", 12, 0, 0, 0)}


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), rounds=[float(x) for x in v])


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])


def keyword(which):
    mode, value, average, wl, wlhat = VARIANTS[which]
    tail = "%d %d %d" % (average, wl, wlhat) if (wl or wlhat) else "%d" % average
    return "compute_orientorder %d %s %g %d %s %s" % (INTERVAL, mode, value, len(DEGREES), " ".join(str(l) for l in DEGREES), tail)


def handle(eng, which, interval):
    from gpumd_amd.nep import OrientOrder
    mode, value, average, wl, wlhat = VARIANTS[which]
    return OrientOrder(eng, mode, value, DEGREES, average, wl, wlhat, interval=interval)


def in_process(drv, torch, nep, h, typ, x, mass, args, out):
    import helpers as H
    n = len(typ)
    vel = H.maxwell_velocities(mass, 300.0, seed=4)
    dt = 1.0 / H.TIME_UNIT
    model = drv.model(nep)
    res = out["pbte"] = dict(atoms=n, degrees=DEGREES, interval=INTERVAL, steps_per_round=args.steps)

    def fresh(which):
        eng = drv.engine(model, n)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
        o = None
        if which:
            o = handle(eng, which, INTERVAL)
            eng.attach(o)
        eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st, o

    def run(eng, st, steps):
        eng.run_nve(h, st["t"], st["m"], dt, steps, st["x"], st["v"], st["pe"], st["f"], st["w"], thermo_every=steps)

    variants = {"nothing_attached": fresh(None)}
    variants.update({k: fresh(k) for k in VARIANTS})
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
    for which in VARIANTS:
        r = res[which] = dict(keyword=keyword(which))
        r["ms_per_sample_in_the_loop"] = spread([(a - b) * INTERVAL for a, b in zip(ms[which], ms["nothing_attached"])])
        r["added_per_step_percent"] = 100.0 * (res["run_nve_ms_per_step"][which]["median"] / base - 1.0)
        last, total, nn, ns = variants[which][2].read()
        r["samples_in_the_loop"] = ns
        r["mean_members"] = float(nn.mean())
        r["mean_columns"] = [float(v) for v in last.mean(axis=0)]
        print("[pbte] %s: %s ms/step -> %+.1f %% per step, %s ms per sample in the loop; mean members %.2f, mean q4 %.4f q6 %.4f"
              % (keyword(which), fmt(res["run_nve_ms_per_step"][which]), r["added_per_step_percent"], fmt(r["ms_per_sample_in_the_loop"]),
                 r["mean_members"], r["mean_columns"][0], r["mean_columns"][1]))

    # (b) one sample alone
    eng0, st0, _ = variants["nothing_attached"]
    for which in VARIANTS:
        o = handle(eng0, which, 1)
        o.sample(st0["x"], h, (1, 1, 1))
        t = []
        for _ in range(3 * args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o.sample(st0["x"], h, (1, 1, 1))
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        o.close()
        s = res[which]["one_sample"] = spread(t)
        print("[pbte] one sample through nepmi_orient_sample, %s: %s ms" % (keyword(which), fmt(s)))
    for eng, st, o in variants.values():
        if o is not None:
            o.close()
        eng.close()
    del variants
    torch.cuda.empty_cache()


def binaries(args, out):
    import ref_compare as R
    if not os.path.exists(R.REF):
        print("oracle/_ref/gpumd_ref is not built: the reference's cost per sample is not measured")
        out.setdefault("not_measured", []).append("reference binary (not built)")
        return
    steps = args.ref_steps
    samples = steps // INTERVAL
    configs = {"none": ""}
    configs.update({k: keyword(k) + "\n" for k in VARIANTS})
    res = {exe: {k: [] for k in configs} for exe in ("gpumd_ref", "gpumd_mi")}
    base = os.path.join(args.scratch, "orient_cost_runs")
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
                            % (args.reps, args.reps, args.reps, extra, steps))
                r, _ = R.run_binary(exe, d, 600.0)
                if r["rc"] != 0 or r["run_seconds"] is None:
                    raise SystemExit("%s failed on %s: see %s/stdout.txt" % (tag, key, d))
                res[tag][key].append(r["run_seconds"])
                print("  round %d %-9s %-10s %d steps %.3f s" % (rnd, tag, key, steps, r["run_seconds"]), flush=True)
    shutil.rmtree(base, ignore_errors=True)
    o = out["pbte"]["binaries"] = dict(steps=steps, samples=samples, rounds=args.ref_rounds,
                                       note="per sample, both programs also print N rows of text into orientorder.out")
    for tag in res:
        q = {k: spread(v) for k, v in res[tag].items()}
        for which in VARIANTS:
            q["ms_per_sample_" + which] = spread([(a - b) * 1e3 / samples for a, b in zip(res[tag][which], res[tag]["none"])])
        o[tag] = q
        print("[pbte] %-9s none %.3f s (%d steps); ms per sample: %s"
              % (tag, q["none"]["median"], steps, ", ".join("%s %s" % (w, fmt(q["ms_per_sample_" + w])) for w in VARIANTS)))


def samples_only(drv, nep, h, typ, x, args):
    """for a profiler run: a few samples of one variant through nepmi_orient_sample, nothing else"""
    eng = drv.engine(drv.model(nep), len(typ))
    o = handle(eng, args.variant, 1)
    d_x = drv.dev(x)
    for _ in range(args.samples_only):
        o.sample(d_x, h, (1, 1, 1))
    last, _, nn, ns = o.read()
    print("%s: %d samples, mean members %.2f, mean columns %s" % (keyword(args.variant), ns, nn.mean(), last.mean(axis=0)))
    o.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref-steps", type=int, default=50)
    ap.add_argument("--ref-rounds", type=int, default=3)
    ap.add_argument("--samples-only", type=int, default=0)
    ap.add_argument("--variant", choices=sorted(VARIANTS), default="cutoff_all")
    ap.add_argument("--no-binaries", action="store_true")
    ap.add_argument("--scratch", default=os.path.join(ROOT, "bench_out"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_cost.json"))
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
