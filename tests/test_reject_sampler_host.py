"""The rejection samplers' f32 classifier (rust-tracing_amd/csrc/rt_reject.hpp) compiled for the HOST: a stand-alone program built
from the header runs the adversarial candidates of tests/test_gpu_reject_sampler.py (fewer of them), so the error bound is checked
without a GPU."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import reject_helpers as rh

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def reject_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("reject_host") / "reject_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", str(ROOT / "rust-tracing_amd" / "csrc"),
                    "-o", str(exe), str(ROOT / "tests" / "reject_host" / "reject_host.cpp")], check=True)

    def run(draws):
        n, k = draws.shape
        src, dst = exe.parent / "in.bin", exe.parent / "out.bin"
        np.ascontiguousarray(draws, dtype=np.uint64).tofile(src)
        subprocess.run([str(exe), str(k), str(src), str(dst)], check=True)
        raw = np.fromfile(dst, dtype=np.uint8)
        assert raw.size == 2 * n + 8 * n * k
        return raw[:n], raw[n:2 * n], raw[2 * n:].view(np.float64).reshape(n, k)
    return run


@pytest.mark.parametrize("k,what", [(3, "sphere"), (2, "disk")])
def test_host_classifier_on_the_adversarial_band(reject_host, k, what):
    draws = rh.adversarial(100_000, k, seed=20 + k)
    verdict32, exact, coords = reject_host(draws)
    l2 = rh.check(draws, verdict32, exact, coords, f"host {what}")
    rh.check_neighbours_occur(l2, what)
    # the set is ON the surface: the candidates moved by at most 2^12 grid steps are all inside the band
    assert (verdict32 == rh.REJECT_UNCERTAIN).mean() > 0.9
