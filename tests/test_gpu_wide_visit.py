"""The visit of a four-child record (rt_kernel.hip visit_wide) against an exact reference, case by case.

Every scene of 64 primitives or more is walked through four-child records.  A visit loads the record (load_oquad, from global memory
or from the LDS tables), runs the conservative packed f32 slab test on its four boxes (box_quad_f32), decides in integer arithmetic on
float bits which children are entered (wide_verdict) and picks the nearest of them (wide_nearest).  The filter may enter a box that the
exact f64 slab test rejects — a wasted visit — and must never do the reverse: the box could hold the closest hit.
rt_debug_wide_visits runs exactly those device functions on caller-supplied cases; the reference here is plain numpy: the slab test of
src/aabb.rs narrowed axis by axis in f64 (what box_miss_f64 does), and the entry / exit distances in long double.

The generator and the reference need no GPU: tests/test_wide_records.py runs them alone and checks that the generator's shares carry
the floors asserted below, so that no assertion here can pass by having nothing to look at."""
import numpy as np
import pytest

import scene_cases

pytestmark = pytest.mark.gpu

EMPTY_REF = np.uint32(7 << 29)
INTERVALS = ((0.001, np.inf), (0.001, 1.0), (-np.inf, np.inf), (0.5, 0.5000001))  # (as test_f32_box_test_never_misses_what_the_exact_test_enters)
N_BASE = 120_000     # cases per interval and load_oquad form: 4 x 2 x 120 k = 0.96 M visits, + per-case intervals, revisits, the filter share
LD = np.longdouble
# the slack of assertion 5: the reference's own rounding.  A long-double slab distance (b - o) / d is two rounded operations on exact
# inputs, each off by at most eps/2 relative: |t_ref - t| <= |t| ((1 + eps/2)^2 - 1) < 1.5 eps |t|; the max / min over axes adds none.
LD_EPS = np.finfo(LD).eps
def ref_slack(t_abs_max): return 1.5 * LD_EPS * t_abs_max


# ---- the generator -----------------------------------------------------------------------------------------------------------------
def gen_cases(n, seed, aimed=True):
    """n cases of (ray, four boxes, references, todo).  aimed: rays through faces, edges, corners and the inside of one of the case's
    boxes, plus the adversarial directions and origins; not aimed: rays towards a random point around the boxes (the filter share)."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2, 3.5, (n, 1, 1))
    lo = rng.uniform(-1, 1, (n, 4, 3)) * scale
    hi = lo + rng.uniform(1e-4, 1, (n, 4, 3)) * scale * rng.choice([1e-3, 1.0], (n, 4, 1))
    # nested and identical boxes in several slots (keys tie), flat boxes (lo == hi on an axis)
    mode = rng.choice(3, n, p=[0.6, 0.2, 0.2])  # 0: four independent boxes, 1: copies of slot 0, 2: nested inside slot 0
    same = (mode == 1)[:, None] & (rng.random((n, 4)) < 0.7)
    lo = np.where(same[:, :, None], lo[:, :1], lo); hi = np.where(same[:, :, None], hi[:, :1], hi)
    shrink = rng.choice([0.0, 0.25, 0.5], (n, 4, 3)) * (hi[:, :1] - lo[:, :1])
    nest = (mode == 2)[:, None] & (rng.random((n, 4)) < 0.7)
    nest[:, 0] = False
    lo = np.where(nest[:, :, None], lo[:, :1] + shrink * rng.choice([0.0, 1.0], (n, 4, 3)), lo)
    hi = np.where(nest[:, :, None], hi[:, :1] - shrink * rng.choice([0.0, 1.0], (n, 4, 3)), hi)
    flat = rng.random((n, 4, 3)) < 0.03
    hi = np.maximum(np.where(flat, lo, hi), lo)  # (a box nested down to nothing on an axis is flat, not inside out)
    # 0-3 empty slots in random positions
    n_empty = rng.choice(4, n, p=[0.4, 0.25, 0.2, 0.15])
    empty = np.argsort(rng.random((n, 4)), axis=1) < n_empty[:, None]
    kinds = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint32), (n, 4))  # inner record / spheres / quads / instance
    refs = (kinds << np.uint32(29)) | rng.integers(0, 1 << 20, (n, 4)).astype(np.uint32)
    refs = np.where(empty, EMPTY_REF, refs).astype(np.uint32)
    # the ray: aimed at a point of one of the boxes that exist (any slot: the second half of the record gets its share)
    aim = np.argmax(rng.random((n, 4)) * ~empty, axis=1)
    alo, ahi = lo[np.arange(n), aim], hi[np.arange(n), aim]
    sc = scale[:, 0]
    o = rng.uniform(-1.5, 1.5, (n, 3)) * sc
    if aimed:
        u = rng.choice([0.0, 1.0, 0.5, 0.25], (n, 3), p=[0.3, 0.3, 0.2, 0.2])
    else:
        u = rng.uniform(-1.0, 2.0, (n, 3))
    target = alo + u * (ahi - alo)
    if aimed:
        inside = rng.random(n) < 0.1                                           # origin inside the box aimed at
        o = np.where(inside[:, None], alo + rng.uniform(0.05, 0.95, (n, 3)) * (ahi - alo), o)
        o = np.where(rng.random((n, 3)) < 0.1, alo, o)                         # origin exactly on a slab plane
    d = target - o
    if aimed:
        d = np.where((rng.random(n) < 0.1)[:, None], -d, d)                    # the box lies behind the origin: negative distances
        d *= 10.0 ** rng.uniform(-3, 3, (n, 1))
        ax = rng.integers(0, 3, n)
        pick = lambda p: (rng.random(n) < p)[:, None] & (np.arange(3)[None, :] == ax[:, None])
        d = np.where(pick(0.05), 0.0, d)                                       # axis-parallel
        d = np.where((rng.random(n) < 0.02)[:, None], d * 1e-300, d)           # 1/d overflows f32
        big = rng.choice([1.0, -1.0], (n, 1)) * 10.0 ** rng.uniform(36, 40, (n, 1))
        d = np.where(pick(0.03), big, d)                                       # 1/d underflows f32, or d itself overflows it
        d = np.where(pick(0.01), 1e300, d)
        d = d * (1.0 + rng.integers(-4, 5, (n, 3)) * 2.0 ** -52)
    todo = rng.integers(0, 16, n).astype(np.uint8) if aimed else np.full(n, 15, dtype=np.uint8)
    lo = np.where(empty[:, :, None], np.inf, lo); hi = np.where(empty[:, :, None], -np.inf, hi)
    boxes = np.stack([lo, hi], axis=-1)  # (n, 4, 3, 2)
    return dict(rays=np.concatenate([o, d], axis=1), boxes=boxes, refs=refs, todo=todo, empty=empty, aim=aim)


def todo_bits(todo):
    return ((todo[:, None] >> np.arange(4, dtype=np.uint8)) & 1).astype(bool)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def ref_enters(rays, boxes, tmin, tmax):
    """src/aabb.rs AABB::hit with the interval narrowed axis by axis, as box_miss_f64 evaluates it: (n, 4) bool."""
    n = rays.shape[0]
    o, d = rays[:, :3], rays[:, 3:]
    lo_t = np.repeat(np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,))[:, None], 4, axis=1)
    hi_t = np.repeat(np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))[:, None], 4, axis=1)
    alive = np.ones((n, 4), dtype=bool)
    with np.errstate(all="ignore"):
        for ax in range(3):
            inv = (1.0 / d[:, ax])[:, None]
            t0 = (boxes[:, :, ax, 0] - o[:, ax, None]) * inv
            t1 = (boxes[:, :, ax, 1] - o[:, ax, None]) * inv
            neg = inv < 0.0
            t0, t1 = np.where(neg, t1, t0), np.where(neg, t0, t1)
            lo_t = np.fmax(t0, lo_t)  # (fmax / fmin: the operand that is not a NaN, as the device's)
            hi_t = np.fmin(t1, hi_t)
            alive &= ~(hi_t <= lo_t)
    return alive


def ref_distances(rays, boxes):
    """Exact entry and exit distance of the ray's LINE through each box, in long double, and the largest |slab distance| that went
    into them (for the slack): three (n, 4) arrays.  Only meaningful where every direction component is finite and not zero."""
    o, d = rays[:, :3].astype(LD), rays[:, 3:].astype(LD)
    b = boxes.astype(LD)
    with np.errstate(all="ignore"):
        t0 = (b[..., 0] - o[:, None, :]) / d[:, None, :]
        t1 = (b[..., 1] - o[:, None, :]) / d[:, None, :]
        near, far = np.minimum(t0, t1), np.maximum(t0, t1)
        mag = np.maximum(np.abs(t0), np.abs(t1)).max(axis=2)
    return near.max(axis=2), far.min(axis=2), mag


def surely_degenerate(rays):
    """Rays that make_ray_pair32 must flag whatever v_rcp_f32 does with denormals: a direction component that is zero, beyond the
    f32 range, or so small that its reciprocal is."""
    a = np.abs(rays[:, 3:])
    return ((a == 0.0) | (a > 3.41e38) | (a < 2.9e-39)).any(axis=1)


# ---- the assertions ----------------------------------------------------------------------------------------------------------------
def check_visits(c, out, tmin, tmax, what, distances=True):
    """Assertions 1-6 on one call's cases; returns the counts the floors are held against."""
    n = len(c["rays"])
    exists, todo = ~c["empty"], todo_bits(c["todo"])
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,)); tmax = np.broadcast_to(np.asarray(tmax, dtype=np.float64), (n,))
    want = ref_enters(c["rays"], c["boxes"], tmin, tmax)
    hit, deg, en, le, chosen = out["hit"], out["degenerate"], out["enter"], out["leave"], out["chosen"]
    show = lambda bad: (what, int(bad.sum()), c["rays"][bad][:2].tolist(), c["boxes"][bad][:2].tolist(), c["todo"][bad][:2].tolist(),
                        en[bad][:2].tolist(), le[bad][:2].tolist(), tmin[bad][:2].tolist(), tmax[bad][:2].tolist())
    # 1. the device's exact verdict is the reference's, slot for slot
    bad = (out["exact"] != want).any(axis=1)
    assert not bad.any(), ("exact verdict",) + show(bad)
    # 2. superset per slot: what the reference enters, of the slots that exist and are to be looked at, is in the hit mask
    must = want & exists & todo
    bad = (must & ~hit).any(axis=1)
    assert not bad.any(), ("a box the exact test enters was culled",) + show(bad)
    # 3. empty slots and slots outside todo are never hit
    bad = (hit & ~(exists & todo)).any(axis=1)
    assert not bad.any(), ("an empty or masked-out slot was entered",) + show(bad)
    # 4. degenerate rays enter every slot that exists and is to be looked at
    bad = deg & (hit != (exists & todo)).any(axis=1)
    assert not bad.any(), ("degenerate ray",) + show(bad)
    bad = surely_degenerate(c["rays"]) & ~deg
    assert not bad.any(), ("a ray with a zero or out-of-range direction component is not flagged",) + show(bad)
    # 5. distance bounds: enter never above max(exact entry, tmin), leave never below min(exact exit, tmax); no NaN
    finite = np.isfinite(c["rays"]).all(axis=1)
    assert not (np.isnan(en) | np.isnan(le))[finite & ~deg].any(), ("NaN distance",) + show(finite & ~deg & (np.isnan(en) | np.isnan(le)).any(axis=1))
    checked = 0
    if distances:
        entry, exit_, mag = ref_distances(c["rays"], c["boxes"])
        ok = (~deg)[:, None] & exists
        with np.errstate(all="ignore"):
            slack = ref_slack(mag)
            too_late = ok & (en.astype(LD) > np.maximum(entry, tmin[:, None].astype(LD)) + slack)
            too_early = ok & (le.astype(LD) < np.minimum(exit_, tmax[:, None].astype(LD)) - slack)
        assert not too_late.any(), ("enter above the exact entry",) + show(too_late.any(axis=1))
        assert not too_early.any(), ("leave below the exact exit",) + show(too_early.any(axis=1))
        checked = int(ok.sum())
    # 6. choice: a hit slot whose enter is the minimum over the hit slots (as floats: -0.0 == 0.0); none iff nothing is hit
    any_hit = hit.any(axis=1)
    assert ((chosen >= 0) == any_hit).all() and (chosen <= 3).all(), ("chosen slot",) + show((chosen >= 0) != any_hit)
    rows = np.flatnonzero(any_hit)
    ch = chosen[rows].astype(np.int64)
    assert hit[rows, ch].all(), ("the chosen slot is not hit",) + show(np.isin(np.arange(n), rows[~hit[rows, ch]]))
    nd = rows[~deg[rows]]  # (a degenerate ray goes on with any of its slots)
    with np.errstate(invalid="ignore"):
        nearest = np.where(hit[nd], en[nd], np.float32(np.inf)).min(axis=1)
        bad_rows = nd[~(en[nd, chosen[nd].astype(np.int64)] == nearest)]
    assert bad_rows.size == 0, ("the chosen slot is not the nearest",) + show(np.isin(np.arange(n), bad_rows))
    ties = int(((np.where(hit[nd], en[nd], np.float32(np.inf)) == nearest[:, None]).sum(axis=1) >= 2).sum())
    return dict(second_half=int(must[:, 2:].sum()), empty_tested=int((c["empty"] & todo).sum()), degenerate=int(deg.sum()),
                degenerate_with_empty=int((deg[:, None] & c["empty"] & todo).sum()), distances=checked, ties=ties, chose=int(any_hit.sum()),
                chose_second_half=int((ch >= 2).sum()), rejected=int((exists & todo & ~hit).sum()), ref_rejected=int((exists & todo & ~want).sum()))


def run(rt, c, tmin, tmax, lds, **kw):
    return rt.debug_wide_visits(c["rays"], tmin, tmax, c["todo"], boxes=c["boxes"], refs=c["refs"], lds=lds, **kw)


def expected_floors(n):
    """Floors on what one call of n generated cases exercises: half the generator's shares, which tests/test_wide_records.py counts
    with the reference alone.  Reference-entered slots in the second half of the record: 0.12 n at (0.001, 1), more at the wider
    intervals; empty slots that are in todo: 1.05 empty slots a case, half the masks have each: 0.55 n; rays with a zero, huge or
    tiny direction component: 0.18 n."""
    return dict(second_half=0.06 * n, empty_tested=0.27 * n, degenerate=0.09 * n)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [0, 1], ids=["global_records", "lds_tables"])
def test_wide_visit_never_culls_what_the_exact_test_enters(rt, gpu, lds):
    """Assertions 1-6 over the four intervals, with load_oquad reading the 256-byte records or the staged LDS tables."""
    c = gen_cases(N_BASE, 2024)
    total = {}
    for tmin, tmax in INTERVALS:
        got = check_visits(c, run(rt, c, tmin, tmax, lds), tmin, tmax, (lds, tmin, tmax))
        floors = expected_floors(N_BASE)
        if (tmin, tmax) != (0.5, 0.5000001):  # (next to nothing is entered within that sliver of an interval)
            assert got["second_half"] > floors["second_half"], (tmin, tmax, got)
        assert got["empty_tested"] > floors["empty_tested"] and got["degenerate"] > floors["degenerate"], (tmin, tmax, got)
        assert got["degenerate_with_empty"] > 0.01 * N_BASE and got["distances"] > 2 * N_BASE, (tmin, tmax, got)
        for k, v in got.items():
            total[k] = total.get(k, 0) + v
    # ties (identical boxes in several slots) and choices in the second half of the record were seen
    assert total["ties"] > 0.01 * 4 * N_BASE and total["chose_second_half"] > 0.03 * 4 * N_BASE, total


def test_wide_visit_with_an_interval_ending_at_a_box(rt, gpu):
    """Per-case intervals (0.001, tmax) with tmax at, and a few f32 ulps around, the exact entry or exit distance of one of the
    case's boxes: the clamp of leave[] to the interval's end decides the verdict."""
    n = 100_000
    c = gen_cases(n, 77)
    rng = np.random.default_rng(78)
    entry, exit_, _ = ref_distances(c["rays"], c["boxes"])
    with np.errstate(all="ignore"):
        at = np.where(rng.random(n) < 0.5, entry[np.arange(n), c["aim"]], exit_[np.arange(n), c["aim"]]).astype(np.float64)
        f = at.astype(np.float32)
        tmax = np.where(rng.random(n) < 0.3, at, (f + rng.integers(-3, 4, n) * np.spacing(np.abs(f))).astype(np.float64))
    tmax = np.where(np.isfinite(tmax), tmax, 1.0)
    at_box = 0
    for lds in (0, 1):
        got = check_visits(c, run(rt, c, 0.001, tmax, lds), 0.001, tmax, ("interval at a box", lds))
        assert got["second_half"] > 0.01 * n and got["ref_rejected"] > 0.2 * n, got
        at_box += got["distances"]
    assert at_box > 2 * n


def test_wide_revisit_keeps_what_the_exact_test_still_enters(rt, gpu):
    """Assertion 7, the rule the set-aside entries rely on.  A record is visited at (0.001, tmax); it is set aside with the mask of
    the children hit other than the chosen one; when its turn comes tmax has shrunk.  The revisit looks at nothing outside that mask,
    and drops none of its children that the exact test still enters at the smaller tmax."""
    n = 150_000
    c = gen_cases(n, 4711)
    rng = np.random.default_rng(4712)
    entry, exit_, _ = ref_distances(c["rays"], c["boxes"])
    dropped = ref_dropped = revisits = kept_second_half = 0
    for lds in (0, 1):
        for tmax in (np.inf, 10.0 ** rng.uniform(-1, 2, n)):
            first = run(rt, c, 0.001, tmax, lds)
            check_visits(c, first, 0.001, tmax, ("first visit", lds), distances=False)
            rest = first["hit"].copy()
            rows = np.flatnonzero(first["chosen"] >= 0)
            rest[rows, first["chosen"][rows].astype(np.int64)] = False
            again = dict(c); again["todo"] = (rest * (1 << np.arange(4))).sum(axis=1).astype(np.uint8)
            # the smaller tmax: where the ray enters or leaves one of the children set aside (exactly, or a few f32 ulps off), or any
            # fraction of the interval
            k = np.argmax(rng.random((n, 4)) * rest, axis=1)
            with np.errstate(all="ignore"):
                at = np.where(rng.random(n) < 0.5, entry[np.arange(n), k], exit_[np.arange(n), k]).astype(np.float64)
                f = at.astype(np.float32)
                near = np.where(rng.random(n) < 0.3, at, (f + rng.integers(-3, 4, n) * np.spacing(np.abs(f))).astype(np.float64))
                frac = entry[np.arange(n), k].astype(np.float64) * rng.uniform(0.2, 1.2, n)  # (mostly short of that child: it must go)
            tmax2 = np.where((rng.random(n) < 0.4) & np.isfinite(near), near, frac)
            sel = rest.any(axis=1) & (tmax2 < tmax) & (tmax2 > 0.001)
            sub = {key: again[key][sel] for key in ("rays", "boxes", "refs", "todo", "empty", "aim")}
            second = run(rt, sub, 0.001, tmax2[sel], lds)
            # hit(tmax') inside todo', and a superset of the reference's verdict at tmax' within todo': assertions 2 and 3 with todo'
            got = check_visits(sub, second, 0.001, tmax2[sel], ("revisit", lds))
            assert not (second["hit"] & ~rest[sel]).any()
            revisits += int(sel.sum()); dropped += int((rest[sel].sum(axis=1) > second["hit"].sum(axis=1)).sum())
            kept_second_half += got["second_half"]; ref_dropped += got["ref_rejected"]
    # Shares of the generator, counted with the reference alone: a first visit enters two or more children in an eighth of the cases
    # and three quarters of the smaller tmax drawn fall inside (0.001, tmax): 0.3 n revisits over the four passes; 60 % of them
    # are drawn at 0.2 .. 1.2 of a set-aside child's entry distance, which the reference then rejects (0.3 n rejected slots), and the
    # filter with it unless tmax' is within its slack of the entry; 0.06 n slots of the second half are still entered.  Floors: half.
    assert revisits > 0.15 * n and ref_dropped > 0.15 * n and dropped > 0.05 * n and kept_second_half > 0.03 * n, (revisits, ref_dropped, dropped, kept_second_half)


def test_wide_visit_is_a_filter(rt, gpu):
    """Assertion 8: on rays that are not aimed at a face, edge or corner the four-slot test rejects practically everything the exact
    test rejects (the floor box_pair_f32 is held to: the arithmetic is the same)."""
    n = 400_000
    c = gen_cases(n, 99, aimed=False)
    for lds in (0, 1):
        got = check_visits(c, run(rt, c, 0.001, np.inf, lds), 0.001, np.inf, ("filter", lds))
        slots = int((~c["empty"]).sum())
        assert got["ref_rejected"] > 0.2 * slots, (got, slots)
        assert got["rejected"] > 0.99 * got["ref_rejected"], got


def test_named_regression_cases(rt, gpu):
    """Hand-written cases that pin corners of the verdict and the choice; a failure found by the random tests is added here."""
    inf = np.inf
    unit = [[0.0, 1.0]] * 3
    empty_box = [[inf, -inf]] * 3
    cases = [
        # ray, boxes, todo, (tmin, tmax), expected hit mask, expected chosen slot
        ("all four identical: lowest slot", [-1, .5, .5, 1, 0, 0], [unit] * 4, 15, (0.001, inf), 15, 0),
        ("identical, slot 0 masked out", [-1, .5, .5, 1, 0, 0], [unit] * 4, 14, (0.001, inf), 14, 1),
        ("only the last slot exists", [-1, .5, .5, 1, 0, 0], [empty_box] * 3 + [unit], 15, (0.001, inf), 8, 3),
        ("empty slots under the universe interval", [-1, .5, .5, 1, 0, 0], [empty_box, unit, empty_box, empty_box], 15, (-inf, inf), 2, 1),
        ("axis-parallel ray: every slot that exists", [5, 5, 5, 0, 1, 0], [unit, empty_box, unit, empty_box], 15, (0.001, inf), 5, None),
        ("infinite direction component", [5, 5, 5, 1, 1e300, 1], [unit, empty_box, unit, unit], 13, (-inf, inf), 13, None),
        ("nothing to look at", [-1, .5, .5, 1, 0, 0], [unit] * 4, 0, (0.001, inf), 0, -1),
        ("box behind the origin", [3, .5, .5, 1, 0.001, 0.001], [unit] * 4, 15, (0.001, inf), 0, -1),
        ("negative distances under the universe interval", [3, .5, .5, 1, 1e-9, 1e-9], [unit] * 4, 15, (-inf, inf), 15, 0),
        ("nearer box in the second half", [-1, .5, .5, 1, 1e-9, 1e-9], [[[2, 3], [0, 1], [0, 1]], empty_box, [[1, 3], [0, 1], [0, 1]], [[0, 1], [0, 1], [0, 1]]], 15, (0.001, inf), 13, 3),
        ("interval ends before the far box", [-1, .5, .5, 1, 1e-9, 1e-9], [[[2, 3], [0, 1], [0, 1]], unit, empty_box, empty_box], 3, (0.001, 2.5), 2, 1),
    ]
    for lds in (0, 1):
        for what, ray, boxes, todo, (tmin, tmax), want_hit, want_chosen in cases:
            b = np.array(boxes, dtype=np.float64).reshape(1, 4, 3, 2)
            out = rt.debug_wide_visits(np.array([ray], dtype=np.float64), tmin, tmax, np.array([todo], dtype=np.uint8), boxes=b, lds=lds)
            got_hit = int((out["hit"][0] * (1 << np.arange(4))).sum())
            assert got_hit == want_hit, (what, lds, got_hit, out)
            if want_chosen is not None:
                assert int(out["chosen"][0]) == want_chosen, (what, lds, out)
            else:
                assert out["degenerate"][0] and out["hit"][0][int(out["chosen"][0])], (what, lds, out)


@pytest.mark.parametrize("name", ["c2_random_balls_96x64_8spp_d50", "c4_final_scene_64x64_8spp_d40", "c3_cornell_box_64x64_16spp_d50"])
def test_wide_visit_on_the_compilers_own_records(rt, gpu, name):
    """Assertion 9: every record the scene compiler makes for the scene (its real empty slots, its real B), through the packed
    images scene creation uploads, against camera rays and random rays.  The reference works on the f32 slot boxes widened to f64."""
    hs = scene_cases.build(rt, name)
    rec = rt.debug_wide_records(hs, wide=1, walk=rt.RT_WALK_OWN_TREES)
    assert rec["wide"]
    n_rec = len(rec["boxes"])
    rng = np.random.default_rng(len(name))
    per = max(64, 200_000 // n_rec)
    n = n_rec * per
    record = np.repeat(np.arange(n_rec, dtype=np.uint32), per)
    boxes = rec["boxes"].astype(np.float64)[record]
    empty = ((rec["refs"] >> 29) == 7)[record]
    cam = hs.camera
    center = np.array(cam.center.tuple())
    p00, du, dv = (np.array(v.tuple()) for v in (cam.pixel00_loc, cam.pixel_delta_u, cam.pixel_delta_v))
    px = p00 + rng.uniform(0, cam.image_width, (n, 1)) * du + rng.uniform(0, cam.image_height, (n, 1)) * dv
    o = np.broadcast_to(center, (n, 3)).copy()
    d = px - o
    # the other half: from a point near the record's boxes towards a point of one of its boxes (corner, edge, face, inside), as
    # scattered rays are; some axis-parallel
    exists = ~empty
    k = np.argmax(rng.random((n, 4)) * exists, axis=1)
    b = boxes[np.arange(n), k]
    size = np.maximum((b[:, :, 1] - b[:, :, 0]).max(axis=1, keepdims=True), 1e-3)
    scattered = (rng.random(n) < 0.5) & exists.any(axis=1)
    o2 = b[:, :, 0] + rng.uniform(-3, 4, (n, 3)) * size
    t2 = b[:, :, 0] + rng.choice([0.0, 1.0, 0.5, 0.25], (n, 3)) * (b[:, :, 1] - b[:, :, 0])
    d2 = (t2 - o2) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    d2 = np.where((rng.random((n, 1)) < 0.05) & (np.arange(3)[None, :] == rng.integers(0, 3, (n, 1))), 0.0, d2)
    o = np.where(scattered[:, None], o2, o); d = np.where(scattered[:, None], d2, d)
    c = dict(rays=np.concatenate([o, d], axis=1), boxes=boxes, refs=rec["refs"][record], todo=rng.integers(0, 16, n).astype(np.uint8),
             empty=empty, aim=k)
    assert np.abs(boxes[exists]).max() <= rec["box_extent"]
    for lds in (0, 1):
        for tmin, tmax in ((0.001, np.inf), (-np.inf, np.inf), (0.001, 10.0 ** rng.uniform(-1, 3, n))):
            out = rt.debug_wide_visits(c["rays"], tmin, tmax, c["todo"], records=rec, record=record, extent=rec["box_extent"], lds=lds)
            got = check_visits(c, out, tmin, tmax, (name, lds))
            assert got["distances"] > n and got["chose"] > 0.05 * n and got["degenerate"] > 0.01 * n, got
            if n_rec > 8:
                assert got["second_half"] > 0.01 * n and got["empty_tested"] > 0, got
