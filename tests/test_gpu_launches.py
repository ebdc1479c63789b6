"""Renders that take SEVERAL launches, at small frames: a 1 MiB sample buffer (RT_SAMPLE_BUFFER_MB=1) makes launch_render
(rt_api.cpp) cut a few dozen samples of a 64x64 frame into chunks, pipelined over two scratch sets and two streams (RT_OVERLAP=1)
or one after the other (RT_OVERLAP=0).  Dense frames, tile shards, list mode with its squared sums, the caller's own accumulate on
top of the chunks, and adaptive batches all go through that loop; all are held to the CPU oracle bit for bit, and
rt_debug_last_launch must report the launch count that the loop's arithmetic gives (at least 3: a case that ran as one launch fails).

Both switches are read when the library loads, so each setting renders in a child process of its own; the parent computes the
oracle's frames and a child never loads the oracle.  The squared sums are the sequential q = q + c * c over the oracle's
single-sample frames, and so are the sums (the oracle's own range render is checked against them once per case).

Not reached here: the out-of-memory back-off of the sample buffer (Workspace::sample_budget) — it needs a real allocation failure,
which a test on a shared machine must not provoke.

Added GPU time, measured on an MI355X: about 17 s for the file (8 child processes: 2 to 3.5 s each of the six main cases)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import scene_cases
from adaptive_helpers import PAD, SENTINEL, assert_bits, bits, launches_for, pad64, replay_schedule, tile_order

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BUDGET = 1 << 20
SEED = 3
N_DENSE, N_SPLIT = 23, 9             # the dense frame and the full list: [0, 23), and [0, 9) + [9, 23) with accumulate
ADAPTIVE = dict(min_spp=22, batch=11, max_spp=43, rel=0.1, abs=0.01)  # points 22, 33, 43
# (case, samples of the shards and of the listed third: enough for three launches of their short sample rows without pipelining)
CASES = [("c2_random_balls_96x64_8spp_d50", 43), ("c3_cornell_box_64x64_16spp_d50", 65), ("c4_final_scene_64x64_8spp_d40", 65)]

CHILD = r"""
import importlib, json, sys
import numpy as np
import torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import scene_cases
rt = importlib.import_module("rust-tracing_amd")
name, out, n_dense, n_split, n_big, seed = sys.argv[2], sys.argv[3], *map(int, sys.argv[4:8])
adaptive = json.loads(sys.argv[8])
hs = scene_cases.build(rt, name)
ds = rt.DeviceScene(hs)
w, h = hs.width, hs.height
stream = torch.cuda.current_stream().cuda_stream
launches, arrays = {}, {}
sentinel = int(np.load(out + ".sentinel.npy")[0])

def note(key):
    launches.setdefault(key, []).append(rt.debug_last_launch()["launches"])

def dense(key, ranges):
    d = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    for b, e in ranges:
        ds.render_device(rt.render_params(seed=seed, sample_begin=b, sample_end=e, accumulate=b > 0), d.data_ptr(), stream)
        note(key)
    torch.cuda.synchronize()
    arrays[key] = d.cpu().numpy()

def shards(key, n, count):
    stride = rt.out_size(w, h, rt.RT_OUT_TILES, 0, count)
    gathered = torch.zeros(count * stride, dtype=torch.float64, device="cuda")
    for r in range(count):
        ds.render_device(rt.render_params(seed=seed, sample_end=n, shard_index=r, shard_count=count, out_layout=rt.RT_OUT_TILES),
                         gathered[r * stride:].data_ptr(), stream)
        note(key)
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    rt.tiles_to_frame_device(w, h, count, gathered.data_ptr(), frame.data_ptr(), stream)
    torch.cuda.synchronize()
    arrays[key] = frame.cpu().numpy()

def listed(key, pixels, ranges):
    lst = torch.from_numpy(pixels.view(np.int32)).cuda()
    s = torch.full((w * h * 3,), sentinel, dtype=torch.int64, device="cuda").view(torch.float64)
    q = torch.full((w * h * 3,), sentinel, dtype=torch.int64, device="cuda").view(torch.float64)
    for b, e in ranges:
        ds.render_pixels_device(rt.render_params(seed=seed, sample_begin=b, sample_end=e, accumulate=b > 0), lst.data_ptr(), len(pixels),
                                s.data_ptr(), q.data_ptr(), stream)
        note(key)
    torch.cuda.synchronize()
    arrays[key + ".sum"], arrays[key + ".sq"] = s.cpu().numpy(), q.cpu().numpy()

dense("dense", [(0, n_dense)])
dense("dense.split", [(0, n_split), (n_split, n_dense)])
shards("shards", n_big, 3)
full, third = np.load(out + ".full.npy"), np.load(out + ".third.npy")
listed("list.full", full, [(0, n_dense)])
listed("list.full.split", full, [(0, n_split), (n_split, n_dense)])
listed("list.third", third, [(0, n_big)])
listed("list.third.split", third, [(0, n_split), (n_split, n_big)])
a = adaptive
total, spp, sq, res = ds.render_adaptive(rt.render_params(seed=seed, sample_end=a["max_spp"]), min_spp=a["min_spp"], batch_spp=a["batch"],
                                         rel=a["rel"], abs=a["abs"])
note("adaptive")
arrays["adaptive.sum"], arrays["adaptive.spp"], arrays["adaptive.sq"] = total, spp, sq
total, spp, sq, one = ds.render_adaptive(rt.render_params(seed=seed, sample_end=a["min_spp"]), min_spp=a["min_spp"], batch_spp=a["batch"],
                                         rel=a["rel"], abs=a["abs"])
note("adaptive.first")
arrays["first.sum"], arrays["first.spp"], arrays["first.sq"] = total, spp, sq
np.savez(out + ".npz", **arrays)
print(json.dumps({"launches": launches, "adaptive": res, "first": one}))
"""

SINGLE = r"""
import ctypes as C, importlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import scene_cases
rt = importlib.import_module("rust-tracing_amd")
name, out, width, spp, seed = sys.argv[2], sys.argv[3], *map(int, sys.argv[4:7])
hs = scene_cases.build(rt, name, width=width)
ds = rt.DeviceScene(hs)
frame = np.full(hs.width * hs.height * 3, -1.0)
params = rt.render_params(seed=seed, sample_end=spp)
rc = rt.amd_lib().rt_render(ds._handle, C.byref(hs.camera), C.byref(params), frame.ctypes.data_as(C.POINTER(C.c_double)))
np.save(out + ".npy", frame)
print(json.dumps({"rc": rc, "error": rt.amd_lib().rt_last_error().decode() if rc else "", "launches": rt.debug_last_launch()["launches"]}))
"""


def run_child(script, overlap, *args):
    env = dict(os.environ, RT_SAMPLE_BUFFER_MB="1", RT_OVERLAP=str(overlap))
    r = subprocess.run([sys.executable, "-c", script, str(ROOT), *map(str, args)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (args, overlap, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def oracle_prefixes(rt, oracle, hs, n):
    """sums[k], squares[k] (n_pix, 3) after k = 0 .. n samples: sequential over the oracle's single-sample frames"""
    n_pix = hs.width * hs.height
    s, q = np.zeros(n_pix * 3), np.zeros(n_pix * 3)
    sums, squares = [s.reshape(n_pix, 3)], [q.reshape(n_pix, 3)]
    for k in range(n):
        c = oracle.render(hs, rt.render_params(seed=SEED, sample_begin=k, sample_end=k + 1))
        s = s + c
        q = q + c * c
        sums.append(s.reshape(n_pix, 3))
        squares.append(q.reshape(n_pix, 3))
    return sums, squares


def third_of_the_pixels(n_pix):
    g = np.random.default_rng(7)
    chosen = g.choice(n_pix, size=n_pix // 3, replace=False).astype(np.uint32)
    g.shuffle(chosen)
    return chosen, np.insert(chosen, g.integers(0, chosen.size, 11), PAD)  # padding entries anywhere in the list


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("case, n_big", CASES)
def test_renders_of_several_launches_equal_the_oracle(rt, oracle, gpu, tmp_path, case, n_big, overlap):
    hs = scene_cases.build(rt, case)
    w, h = hs.width, hs.height
    n_pix, n_tiles = w * h, ((w + 7) // 8) * ((h + 7) // 8)
    a = ADAPTIVE
    assert n_big >= a["max_spp"]
    sums, squares = oracle_prefixes(rt, oracle, hs, n_big)
    assert_bits(oracle.render(hs, rt.render_params(seed=SEED, sample_end=N_DENSE)).reshape(n_pix, 3), sums[N_DENSE], "oracle: one range against its samples")
    full = tile_order(w, h)
    chosen, third = third_of_the_pixels(n_pix)
    out = str(tmp_path / "child")
    np.save(out + ".full.npy", full)
    np.save(out + ".third.npy", third)
    np.save(out + ".sentinel.npy", np.array([SENTINEL]).view(np.int64))
    stats = run_child(CHILD, overlap, case, out, N_DENSE, N_SPLIT, n_big, SEED, json.dumps(a))
    got = np.load(out + ".npz")
    launches = stats["launches"]
    count = lambda entries, n: launches_for(entries, n, BUDGET, overlap)[0]

    # dense frames and shards
    for key in ("dense", "dense.split"):
        assert_bits(got[key].reshape(n_pix, 3), sums[N_DENSE], f"{case} {key}")
    assert_bits(got["shards"].reshape(n_pix, 3), sums[n_big], f"{case} three shards")
    assert launches["dense"] == [count(n_tiles * 64, N_DENSE)] and launches["dense"][0] >= 3, launches
    assert launches["dense.split"] == [count(n_tiles * 64, N_SPLIT), count(n_tiles * 64, N_DENSE - N_SPLIT)], launches
    assert N_DENSE % launches_for(n_tiles * 64, N_DENSE, BUDGET, overlap)[1] != 0, "the last launch is not ragged"
    assert launches["shards"] == [count((n_tiles - r + 2) // 3 * 64, n_big) for r in range(3)] and min(launches["shards"]) >= 3, launches

    # list mode: sums and squared sums on the listed pixels, the sentinel elsewhere
    mask = np.zeros(n_pix, dtype=bool)
    mask[chosen] = True
    for key, pixels, sel, n in (("list.full", full, np.ones(n_pix, dtype=bool), N_DENSE), ("list.third", third, mask, n_big)):
        for k in (key, key + ".split"):
            s, q = got[k + ".sum"].reshape(n_pix, 3), got[k + ".sq"].reshape(n_pix, 3)
            assert_bits(s[sel], sums[n][sel], f"{case} {k}: sums")
            assert_bits(q[sel], squares[n][sel], f"{case} {k}: squared sums")
            assert (bits(s[~sel]) == SENTINEL).all() and (bits(q[~sel]) == SENTINEL).all(), f"{case} {k}: an unlisted pixel was written"
        assert launches[key] == [count(len(pixels), n)] and launches[key][0] >= 3, (key, launches)
        assert launches[key + ".split"] == [count(len(pixels), N_SPLIT), count(len(pixels), n - N_SPLIT)], (key, launches)
        assert n % launches_for(len(pixels), n, BUDGET, overlap)[1] != 0, "the last launch is not ragged"

    # adaptive: the numpy replay over the oracle's sums; the first batch alone is several launches
    points = list(range(a["min_spp"], a["max_spp"], a["batch"])) + [a["max_spp"]]
    snap, snap_q = {n: sums[n] for n in points}, {n: squares[n] for n in points}
    want_spp, batches, active = replay_schedule(snap, snap_q, points, a["rel"], a["abs"])
    spp = got["adaptive.spp"].reshape(-1)
    assert (spp == want_spp).all(), f"{int((spp != want_spp).sum())} pixels' spp differ from the replay"
    assert np.unique(spp).size >= 2, np.unique(spp)
    total, sq = got["adaptive.sum"].reshape(n_pix, 3), got["adaptive.sq"].reshape(n_pix, 3)
    for n in points:
        sel = spp == n
        assert_bits(total[sel], snap[n][sel], f"{case} adaptive: sums of the pixels that stopped at {n}")
        assert_bits(sq[sel], snap_q[n][sel], f"{case} adaptive: squared sums of the pixels that stopped at {n}")
    assert stats["adaptive"] == {"samples": int(spp.sum()), "launches": batches, "converged": int((spp < a["max_spp"]).sum())}
    last_entries = len(full) if batches == 1 else pad64(active[batches - 1])
    last_samples = points[batches - 1] - (points[batches - 2] if batches > 1 else 0)
    assert launches["adaptive"] == [count(last_entries, last_samples)], (launches, last_entries, last_samples)
    chunk = launches_for(len(full), 1 << 20, BUDGET, overlap)[1]  # samples of the full list that the buffer holds
    assert a["min_spp"] > chunk and a["batch"] % chunk != 0
    assert launches["adaptive.first"] == [count(len(full), a["min_spp"])] and launches["adaptive.first"][0] >= 3, launches
    assert (got["first.spp"] == a["min_spp"]).all() and stats["first"] == {"samples": n_pix * a["min_spp"], "launches": 1, "converged": 0}
    assert_bits(got["first.sum"].reshape(n_pix, 3), sums[a["min_spp"]], f"{case} adaptive, one batch: sums")
    assert_bits(got["first.sq"].reshape(n_pix, 3), squares[a["min_spp"]], f"{case} adaptive, one batch: squared sums")


def test_a_sample_row_of_more_than_half_the_buffer_runs_one_sample_per_launch(rt, oracle, gpu, tmp_path):
    """192x128: 384 tiles, 589 824 bytes per sample row — under the budget, over its half: no pipelining, as many launches as samples"""
    case, width, spp = "c2_random_balls_96x64_8spp_d50", 192, 5
    hs = scene_cases.build(rt, case, width=width)
    entries = ((hs.width + 7) // 8) * ((hs.height + 7) // 8) * 64
    assert BUDGET // 2 < entries * 24 <= BUDGET
    assert launches_for(entries, spp, BUDGET, True) == (spp, 1, False)
    out = str(tmp_path / "child")
    stats = run_child(SINGLE, 1, case, out, width, spp, SEED)
    assert stats["rc"] == 0, stats
    assert stats["launches"] == spp
    assert_bits(np.load(out + ".npy"), oracle.render(hs, rt.render_params(seed=SEED, sample_end=spp)), "one sample per launch")


def test_a_sample_row_larger_than_the_buffer_is_refused_with_a_status(rt, gpu, tmp_path):
    """256x170: 704 tiles, 1 081 344 bytes per sample row: RT_ERR_UNSUPPORTED before anything is launched or written"""
    case, width = "c2_random_balls_96x64_8spp_d50", 256
    hs = scene_cases.build(rt, case, width=width)
    entries = ((hs.width + 7) // 8) * ((hs.height + 7) // 8) * 64
    assert entries * 24 > BUDGET and launches_for(entries, 4, BUDGET, True)[0] == 0
    out = str(tmp_path / "child")
    stats = run_child(SINGLE, 1, case, out, width, 4, SEED)
    assert stats["rc"] == -5, stats  # RT_ERR_UNSUPPORTED
    assert "does not fit the sample buffer" in stats["error"], stats
    assert stats["launches"] == 0
    assert (np.load(out + ".npy") == -1.0).all(), "a refused render wrote to the caller's frame"
