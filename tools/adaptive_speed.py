#!/usr/bin/env python3
"""What adaptive sampling (rt_render_adaptive_device) buys on time-to-image, and what list mode itself costs.  Not part of bench.py.

  C3 (Cornell 600x600, max 1000 spp) and C4 (final_scene 800x800, max 5000 spp): wall time and mean spp of the adaptive render at a
  few relative thresholds and of the uniform render; the RMSE of each against an independent uniform render at max spp (seed 2), and
  the RMSE of a uniform render that takes the adaptive render's wall time.  RMSE of the per-pixel means: linear, and clipped to
  [0, 1] (what the PNG can show).
  List mode's own cost: the full list in tile order (rt_render_pixels_device) against rt_render_device, same spp, C2 and C3.

Usage: python tools/adaptive_speed.py [--out FILE] [--workloads c3 c4] [--rel 0.01 0.02 0.05] [--abs 1e-3] [--schedules 16:16 64:64]
                                      [--reps 3]   (a schedule is min_spp:batch_spp; every schedule is run at every --rel)"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

rt = importlib.import_module("rust-tracing_amd")
EARTH = str(ROOT / "assets" / "earth-large.jpg") if (ROOT / "assets" / "earth-large.jpg").exists() else "synthetic:6400x3200"
WORKLOADS = {  # bench.py's configs
    "c2": dict(scene=0, width=1200, aspect=1.5, spp=500, depth=50),
    "c3": dict(scene=6, width=600, aspect=1.0, spp=1000, depth=50),
    "c4": dict(scene=8, width=800, aspect=1.0, spp=5000, depth=40, earth_image=EARTH),
}


def tile_order(w, h):
    tx, ty = (w + 7) // 8, (h + 7) // 8
    k = np.arange(tx * ty * 64, dtype=np.int64)
    t, p = k >> 6, k & 63
    i, j = (t % tx) * 8 + (p & 7), (t // tx) * 8 + (p >> 3)
    return np.where((i < w) & (j < h), j * w + i, 0xFFFFFFFF).astype(np.uint32)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def uniform(ds, n_pix, spp, seed=1):
    d = torch.zeros(n_pix * 3, dtype=torch.float64, device="cuda")
    dt, _ = timed(lambda: ds.render_device(rt.render_params(seed=seed, sample_end=spp), d.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return dt, (d.view(n_pix, 3) / spp).cpu().numpy()


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2))), float(np.sqrt(np.mean((np.clip(a, 0, 1) - np.clip(b, 0, 1)) ** 2)))


def quality(name, rels, abs_t, schedules, log):
    cfg = WORKLOADS[name]
    hs = rt.HostScene(cfg["scene"], width=cfg["width"], aspect=cfg["aspect"], spp=cfg["spp"], depth=cfg["depth"],
                      earth_image=cfg.get("earth_image"))
    ds = rt.DeviceScene(hs)
    n_pix, max_spp = hs.width * hs.height, cfg["spp"]
    uniform(ds, n_pix, 8)  # warm-up (scratch, code objects: the dense and the list kernels)
    w_sum = torch.zeros(n_pix * 3, dtype=torch.float64, device="cuda")
    w_spp = torch.zeros(n_pix, dtype=torch.int32, device="cuda")
    ds.render_adaptive_device(rt.render_params(seed=1, sample_end=8), rt.adaptive_params(min_spp=4, batch_spp=4), w_sum.data_ptr(), w_spp.data_ptr())
    del w_sum, w_spp
    _, ref = uniform(ds, n_pix, max_spp, seed=2)
    t_uni, img = uniform(ds, n_pix, max_spp)
    rate = n_pix * max_spp / t_uni
    rows = [dict(workload=name, mode="uniform", rel=None, wall_s=t_uni, mean_spp=float(max_spp), rmse=rmse(img, ref))]
    log(f"{name} {hs.width}x{hs.height} max {max_spp} spp: uniform {t_uni:.3f} s ({rate / 1e6:.0f} Msamples/s), RMSE lin {rows[0]['rmse'][0]:.5f} "
        f"clipped {rows[0]['rmse'][1]:.5f} (against an independent {max_spp}-spp render)")
    d_sum = torch.zeros(n_pix * 3, dtype=torch.float64, device="cuda")
    d_spp = torch.zeros(n_pix, dtype=torch.int32, device="cuda")
    for (min_spp, batch_spp), rel in ((sc, rel) for sc in schedules for rel in rels):
        a = rt.adaptive_params(min_spp=min_spp, batch_spp=batch_spp, rel_threshold=rel, abs_threshold=abs_t)
        dt, res = timed(lambda: ds.render_adaptive_device(rt.render_params(seed=1, sample_end=max_spp), a, d_sum.data_ptr(), d_spp.data_ptr(),
                                                          0, torch.cuda.current_stream().cuda_stream))
        spp = d_spp.cpu().numpy()
        img = (d_sum.view(n_pix, 3).cpu().numpy() / spp[:, None])
        mean_spp = res["samples"] / n_pix
        row = dict(workload=name, mode="adaptive", rel=rel, abs=abs_t, min_spp=int(a.min_spp), batch_spp=int(a.batch_spp), wall_s=dt,
                   mean_spp=mean_spp, spp_min=int(spp.min()), spp_max=int(spp.max()), launches=res["launches"], converged=res["converged"],
                   rmse=rmse(img, ref))
        # the uniform render that takes the same wall time
        eq_spp = max(1, int(round(dt * rate / n_pix)))
        t_eq, img_eq = uniform(ds, n_pix, eq_spp)
        row.update(equal_time_spp=eq_spp, equal_time_wall_s=t_eq, equal_time_rmse=rmse(img_eq, ref))
        rows.append(row)
        log(f"  min {min_spp:<4d} batch {batch_spp:<4d} rel {rel:<6g} abs {abs_t:g}: {dt:.3f} s, mean {mean_spp:.1f} spp (min {row['spp_min']}, max {row['spp_max']}), "
            f"{res['launches']} launches, {res['converged']} pixels converged; RMSE lin {row['rmse'][0]:.5f} clipped {row['rmse'][1]:.5f}  |  "
            f"uniform at the same time: {eq_spp} spp, {t_eq:.3f} s, RMSE lin {row['equal_time_rmse'][0]:.5f} clipped {row['equal_time_rmse'][1]:.5f}")
    return rows


def list_cost(name, reps, log):
    cfg = WORKLOADS[name]
    hs = rt.HostScene(cfg["scene"], width=cfg["width"], aspect=cfg["aspect"], spp=cfg["spp"], depth=cfg["depth"],
                      earth_image=cfg.get("earth_image"))
    ds = rt.DeviceScene(hs)
    n_pix, spp = hs.width * hs.height, cfg["spp"]
    stream = torch.cuda.current_stream().cuda_stream
    lst = torch.from_numpy(tile_order(hs.width, hs.height).view(np.int32)).cuda()
    a = torch.zeros(n_pix * 3, dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    p = rt.render_params(seed=1, sample_end=spp)
    dense = lambda: ds.render_device(p, a.data_ptr(), stream)
    listed = lambda: ds.render_pixels_device(p, lst.data_ptr(), lst.numel(), b.data_ptr(), 0, stream)
    dense(); listed()  # warm-up
    td, tl = [], []
    for _ in range(reps):  # alternating
        td.append(timed(dense)[0])
        tl.append(timed(listed)[0])
    same = bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))
    md, ml = float(np.median(td)), float(np.median(tl))
    log(f"list mode {name} {hs.width}x{hs.height}x{spp}: rt_render_device {md:.4f} s ({n_pix * spp / md / 1e6:.0f} Msamples/s), "
        f"full list {ml:.4f} s ({n_pix * spp / ml / 1e6:.0f} Msamples/s), ratio {ml / md:.4f}, frames bit-identical: {same}  "
        f"(median of {reps}; dense {['%.4f' % t for t in td]}, list {['%.4f' % t for t in tl]})")
    return dict(workload=name, dense_s=td, list_s=tl, ratio=ml / md, identical=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adaptive_speed.txt"))
    ap.add_argument("--workloads", nargs="*", default=["c3", "c4"])
    ap.add_argument("--rel", nargs="*", type=float, default=[0.01, 0.02, 0.05])
    ap.add_argument("--abs", type=float, default=1e-3)
    ap.add_argument("--schedules", nargs="*", default=["16:16"], help="min_spp:batch_spp pairs (16:16 are the library's defaults)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--list-workloads", nargs="*", default=["c2", "c3"])
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"adaptive_speed on {torch.cuda.get_device_name(0)}")
    data = dict(quality=[], list_mode=[])
    for w in args.list_workloads:
        data["list_mode"].append(list_cost(w, args.reps, log))
    for w in args.workloads:
        data["quality"] += quality(w, args.rel, args.abs, [tuple(int(x) for x in sc.split(":")) for sc in args.schedules], log)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    out.with_suffix(".json").write_text(json.dumps(data, indent=1) + "\n")


if __name__ == "__main__":
    main()
