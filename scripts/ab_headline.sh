#!/bin/bash
# A/B of variant libraries on the headline stream (64x120, 10 k keyframes): scripts/ab_headline.sh NAME... (each variant of
# scl_slam_amd/lib/variants in front of the product library, alternating): three times the default line, twice the driver's form.
# Stops at the first run that fails.
cd "$(dirname "$0")/.."
python3 - "$@" <<'PY'
import json, os, subprocess, sys
names = sys.argv[1:] + ["result"]
for reps, form in ((3, ["--repeats", "5"]), (2, ["--gpus", "1", "--steps", "20", "--warmup", "5"])):
    for rep in range(reps):
        for n in names:
            env = dict(os.environ)
            env.pop("SCL_ENGINE_LIB", None)
            if n != "result": env["SCL_ENGINE_LIB"] = os.path.join("scl_slam_amd/lib/variants", f"libscl_engine_{n}.so")
            out = subprocess.run([sys.executable, "bench.py"] + form, env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(n, "failed with status", out.returncode, out.stderr[-400:], flush=True)
                sys.exit(out.returncode if out.returncode > 0 else 1)
            d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
            print(f"{n:8s} {' '.join(form):40s} value {d['value']/1e9:8.4f} G pairs/s  step {d['ms_per_step']*1e3:7.2f} us  "
                  f"entry {d['kernel_ms']['sc_distance']*1e3:7.2f} us of {d['roofline']['scans_per_launch']:.0f} scans  frac {d['roofline']['frac']:.3f}", flush=True)
PY
