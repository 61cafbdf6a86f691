#!/usr/bin/env python3
"""What sampling the mass-weighted velocity autocorrelation inside the run loop costs, beside the unweighted one: PbTe, 1,024,000
atoms (the 250-atom cell 16 x 16 x 16), NVE, 300 K, 1 fs, one engine per variant, alternating rounds in one process:

  (a) nepmi_run_nve ms/step with nothing attached, with a VAC correlator (`compute_sdc 5 200`) and with an MVAC correlator
      (`compute_dos 5 200 400`) attached; the rounds start after 1000 warm-up steps, so every sample is a time origin and the
      difference x 5 is the cost of one sample (second half-kick as a pass of its own + gather + correlation over 200 lags);
  (b) one sample alone through nepmi_corr_sample on a full ring, quantities 1 and 2, timed with events on the engine's stream,
      against the kernel's compulsory bytes (Nc + 1) n 24 (4.9 GB here; the weights add n 8).

Alternating runs, three rounds, median (min .. max) printed; measured, not asserted.

    python profiles/dos_cost.py [--reps 16] [--steps 500] [--rounds 3] [--swap] [--out profiles/dos_cost.json] [--txt profiles/dos_cost.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
INTERVAL, NC, OMEGA = 5, 200, 400.0
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), rounds=[float(x) for x in v])


def fmt(s):
    return "%.4f (%.4f .. %.4f)" % (s["median"], s["min"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dos_cost.json"))
    ap.add_argument("--txt", default=os.path.join(ROOT, "profiles", "dos_cost.txt"))
    ap.add_argument("--swap", action="store_true", help="create and run the weighted variant before the unweighted one")
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
    say("PbTe %d atoms, NVE, 1 fs; sample interval %d, %d lags; %d rounds of %d steps, alternating" % (n, INTERVAL, NC, args.rounds, args.steps))

    def fresh(quantity):
        eng = drv.engine(model, n)
        st = dict(t=drv.dev(typ), m=drv.dev(mass), x=drv.dev(x), v=drv.dev(vel), pe=drv.zeros(n), f=drv.zeros(3 * n), w=drv.zeros(9 * n))
        corr = None
        if quantity:
            corr = Correlator(eng, quantity, INTERVAL, NC, weights=mass if quantity == "mvac" else None)
            eng.attach(corr)
        eng.force_compute(h, st["t"], st["x"], st["pe"], st["f"], st["w"])
        return eng, st, corr

    def run(eng, st, steps):
        eng.run_nve(h, st["t"], st["m"], dt, steps, st["x"], st["v"], st["pe"], st["f"], st["w"], thermo_every=steps)

    order = [("nothing_attached", None), ("compute_sdc_5_200", "vac"), ("compute_dos_5_200_400", "mvac")]
    if args.swap:
        order[1], order[2] = order[2], order[1]
        say("(the weighted variant is created and run before the unweighted one)")
    variants = {name: fresh(quantity) for name, quantity in order}
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
            s["ms_per_sample"] = spread([(a - b) * INTERVAL for a, b in zip(ms[name], ms["nothing_attached"])])
            s["samples"], s["time_origins"] = samples, origins
            extra = "; per sample %s ms; %d samples, %d time origins" % (fmt(s["ms_per_sample"]), samples, origins)
        say("%-24s %s ms/step%s" % (name, fmt(s), extra))
    a, b = out["run_nve_ms_per_step"]["compute_sdc_5_200"]["ms_per_sample"], out["run_nve_ms_per_step"]["compute_dos_5_200_400"]["ms_per_sample"]
    out["weighted_minus_unweighted_ms_per_sample"] = b["median"] - a["median"]
    out["unweighted_spread_ms_per_sample"] = a["max"] - a["min"]
    say("weighted - unweighted, per sample: %+.4f ms; the unweighted form's own spread (max - min): %.4f ms"
        % (out["weighted_minus_unweighted_ms_per_sample"], out["unweighted_spread_ms_per_sample"]))
    omega, mvac, dos = variants["compute_dos_5_200_400"][2].dos(INTERVAL * 1e-3, OMEGA)
    out["dos_peak_THz"] = [float(omega[np.argmax(dos[0, d])]) for d in range(3)]
    say("(the DOS of that run peaks at omega = %s THz)" % " ".join("%.0f" % v for v in out["dos_peak_THz"]))
    out["describe"] = variants["nothing_attached"][0].describe()

    # (b) one sample on a full ring
    eng, st, _ = variants["nothing_attached"]
    compulsory = (NC + 1) * n * 24
    out["one_sample"] = dict(compulsory_bytes=compulsory)
    for quantity in ("vac", "mvac"):
        c = Correlator(eng, quantity, 1, NC, weights=mass if quantity == "mvac" else None)
        for _ in range(NC + 2):
            c.sample(st["v"])
        t = []
        for _ in range(3 * args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c.sample(st["v"])
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        c.close()
        s = spread(t)
        s["TB_per_s"] = compulsory / (s["median"] * 1e-3) / 1e12
        out["one_sample"][quantity] = s
        say("one %-4s sample alone (gather + %d lags + reduction): %s ms = %.2f TB/s of the %.2f GB it must read"
            % (quantity, NC, fmt(s), s["TB_per_s"], compulsory / 1e9))
    for eng, st, corr in variants.values():
        if corr is not None:
            corr.close()
        eng.close()
    for path, text in ((args.out, json.dumps(out, indent=1)), (args.txt, "\n".join(LINES) + "\n")):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    print("written: %s, %s" % (args.out, args.txt))


if __name__ == "__main__":
    main()
