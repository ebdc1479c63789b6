"""The rejection samplers' accept / reject decision on the device (rust-tracing_amd/csrc/rt_reject.hpp through rt_debug_eval's
RT_DEBUG_REJECT_* ops, which call the functions the render kernel calls): the f32 classifier may say "certain" only where the exact
f64 predicate agrees, the exact predicate and the coordinates built from the kept draws are the reference's bit for bit, and the
classifier leaves next to nothing to the exact predicate."""
import numpy as np
import pytest

import reject_helpers as rh

pytestmark = pytest.mark.gpu


def classify(rt, draws):
    """(f32 verdicts, exact verdicts, coordinates) of candidates given as (n, K) raw draws."""
    n, k = draws.shape
    ops = (rt.RT_DEBUG_REJECT_SPHERE_VERDICTS, rt.RT_DEBUG_REJECT_SPHERE_COORDS) if k == 3 else \
          (rt.RT_DEBUG_REJECT_DISK_VERDICTS, rt.RT_DEBUG_REJECT_DISK_COORDS)
    flat = np.ascontiguousarray(draws, dtype=np.uint64).reshape(-1).view(np.float64)
    verdicts = rt.debug_eval(ops[0], flat).reshape(n, k)
    coords = rt.debug_eval(ops[1], flat).reshape(n, k)
    return verdicts[:, 0].astype(np.int64), verdicts[:, 1].astype(np.int64), coords


@pytest.mark.parametrize("k,n,what", [(3, 1 << 20, "sphere"), (2, 1 << 18, "disk")])
def test_classifier_on_the_adversarial_band(rt, gpu, k, n, what):
    draws = rh.adversarial(n, k, seed=10 + k)
    verdict32, exact, coords = classify(rt, draws)
    l2 = rh.check(draws, verdict32, exact, coords, f"device {what}")
    rh.check_neighbours_occur(l2, what)


def test_the_filter_filters(rt, gpu):
    rng = np.random.default_rng(77)
    n = 1 << 20
    for k, inside, what in ((3, np.pi / 6.0, "sphere"), (2, np.pi / 4.0, "disk")):
        draws = rng.integers(0, 1 << 64, (n, k), dtype=np.uint64)
        verdict32, exact, coords = classify(rt, draws)
        rh.check(draws, verdict32, exact, coords, f"device {what}, uniform draws")
        uncertain = (verdict32 == rh.REJECT_UNCERTAIN).mean()
        accepted = (verdict32 == rh.REJECT_YES).mean()
        print(f"{what}: uncertain {uncertain:.3e}, certain accepts {accepted:.5f} (pi share {inside:.5f})")
        # the band's shell is 4 pi band / 8 of the cube (2 pi band / 4 of the square): a few 1e-6
        assert uncertain <= 1e-4, what
        assert abs(accepted - inside) <= 0.01, what
