"""RT_WIDE_SETASIDE: a four-child record with one child left to look at sets an inner child aside as its own entry (1, the default)
instead of itself with a one-bit mask (0).  Speed only: the frames must be bit-identical to each other and to the oracle, the walk
must visit fewer records, and no record may be revisited only to pick the one inner child left.

The switch is read when the library loads, so each setting renders in a child process of its own."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scene_cases

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

CHILD = r"""
import importlib, json, sys
import numpy as np
import torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import scene_cases
rt = importlib.import_module("rust-tracing_amd")
name, wide, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
hs = scene_cases.build(rt, name)
params = rt.render_params(seed=4)
ds = rt.DeviceScene(hs, wide=wide)
plain = ds.render(params)
d = torch.zeros(hs.width * hs.height * 3, dtype=torch.float64, device="cuda")
cnt = ds.render_device_counted(params, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
np.save(out + ".plain.npy", plain)
np.save(out + ".counted.npy", d.cpu().numpy())
print(json.dumps({"counters": cnt, "visits": rt.debug_visit_stats()}))
"""


def run_child(tmp_path, name, wide, setting):
    out = str(tmp_path / f"{name}_{wide}_{setting}")
    env = dict(os.environ, RT_WIDE_SETASIDE=str(setting))
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), name, str(wide), out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (name, setting, r.returncode, r.stderr[-2000:])
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    return np.load(out + ".plain.npy"), np.load(out + ".counted.npy"), stats["counters"], stats["visits"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# (C3's Cornell box is walked with two-child records by default: four are forced here so that the rule runs on quads and instances too)
@pytest.mark.parametrize("name, wide, fewer", [
    ("c2_random_balls_96x64_8spp_d50", -1, True),
    ("c3_cornell_box_64x64_16spp_d50", 1, False),
    ("c4_final_scene_64x64_8spp_d40", -1, True),
])
def test_setaside_rule_changes_the_walk_not_the_frame(rt, oracle, gpu, tmp_path, name, wide, fewer):
    hs = scene_cases.build(rt, name)
    want = oracle.render(hs, rt.render_params(seed=4))
    plain0, counted0, c0, v0 = run_child(tmp_path, name, wide, 0)
    plain1, counted1, c1, v1 = run_child(tmp_path, name, wide, 1)
    for what, got in (("rule off", plain0), ("rule off, counted", counted0), ("rule on", plain1), ("rule on, counted", counted1)):
        neq = bits(got) != bits(want)
        assert not neq.any(), f"{name} {what}: {int(neq.sum())} of {neq.size} values differ from the oracle"
    for key in ("samples", "rays", "sphere_tests", "quad_tests", "rng_draws"):
        assert c0[key] == c1[key], (name, key, c0[key], c1[key])
    # the walk is a four-child one — every record visit is one of the classified kinds (the Cornell box's may all be revisits: its queries
    # start in the walls' leaf with the root set aside, a box's frame in its faces' leaf) ...
    for c, v in ((c0, v0), (c1, v1)):
        assert c["node_visits"] > 0, name
        assert sum(x for k, x in v.items() if not k.startswith("push.")) == c["node_visits"], (name, c["node_visits"], v)
    # ... and the rule did its work: no record is revisited only to pick the one inner child left
    assert v0["push.child"] == 0 and v1["revisit1.inner"] == 0, (name, v0, v1)
    if fewer:
        assert v0["first"] > 0 and v0["revisit1.inner"] > 0 and v1["push.child"] > 0, (name, v0, v1)
    assert c1["node_visits"] <= c0["node_visits"], (name, c0["node_visits"], c1["node_visits"])
    if fewer:
        assert c1["node_visits"] < c0["node_visits"], (name, c0["node_visits"], c1["node_visits"])
