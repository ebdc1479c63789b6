#!/usr/bin/env python3
"""How the four-child walk spends its record visits: the instrumented kernel's rt_debug_visit_stats for bench workloads, with
RT_WIDE_SETASIDE=0 (a record with one child left is set aside as itself with a one-bit mask) and =1 (an inner child left alone is
set aside as its own entry).  The switch is read when the library loads, so every setting runs in a child process of its own.
Prints, per workload and setting, visits per sample and their split into first visits and revisits (by children left and by what
the walk went on with)."""
import argparse
import importlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def child(workload, spp):
    sys.path.insert(0, str(ROOT))
    import torch
    rt = importlib.import_module("rust-tracing_amd")
    import bench
    wl = dict(bench.WORKLOADS[workload]); wl.pop("name")
    hs = rt.HostScene(wl["scene"], scene_seed=bench.SCENE_SEED, width=wl["width"], aspect=wl["aspect"], spp=spp, depth=wl["depth"],
                      earth_image=wl.get("earth_image"))
    ds = rt.DeviceScene(hs)
    frame = torch.zeros(hs.width * hs.height * 3, dtype=torch.float64, device="cuda")
    cnt = ds.render_device_counted(rt.render_params(seed=bench.RENDER_SEED), frame.data_ptr(), torch.cuda.current_stream().cuda_stream)
    print(json.dumps({"counters": cnt, "visits": rt.debug_visit_stats()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["c2", "c3", "c4"])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--settings", default="0,1", help="RT_WIDE_SETASIDE values to run")
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "SPP"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]))
        return
    for w in args.workloads:
        for setting in args.settings.split(","):
            env = dict(os.environ, RT_WIDE_SETASIDE=setting)
            out = subprocess.run([sys.executable, __file__, "--child", w, str(args.spp)], env=env, capture_output=True, text=True,
                                 timeout=600)
            if out.returncode != 0:
                sys.stderr.write(out.stderr)
                raise SystemExit(f"{w} RT_WIDE_SETASIDE={setting}: exit {out.returncode}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            c, v = r["counters"], r["visits"]
            n = max(1, c["samples"])
            visits = c["node_visits"]
            counted = sum(x for k, x in v.items() if not k.startswith("push."))
            print(f"{w} RT_WIDE_SETASIDE={setting}  {args.spp} spp  node_visits/sample {visits / n:.3f}  (wide visits counted {counted / n:.3f})")
            if counted == 0:
                print("  (no four-child records in this scene's walk)")
                continue
            print(f"  first visits          {v['first'] / n:8.3f} /sample  {100 * v['first'] / counted:5.1f} %")
            for b in (1, 2, 3):
                row = "  ".join(f"{o} {v[f'revisit{b}.{o}'] / n:7.3f} ({100 * v[f'revisit{b}.{o}'] / counted:4.1f} %)" for o in ("inner", "leaf", "none"))
                print(f"  revisits, {b} left     {row}")
            print(f"  set aside: record+mask {v['push.record'] / n:.3f} /sample, child's own entry {v['push.child'] / n:.3f} /sample")
            print(f"  revisits with one inner child left: {100 * v['revisit1.inner'] / counted:.1f} % of visits")


if __name__ == "__main__":
    main()
