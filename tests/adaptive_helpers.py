"""Shared by the adaptive-sampling and multi-launch GPU tests (not a test module): bit-for-bit comparison, the tile-order pixel list,
the convergence rule and one step of the schedule in numpy, launch_render's chunk arithmetic, and the check of rt_render_adaptive
against the CPU oracle at every pixel's own sample count."""
import numpy as np

PAD = 0xFFFFFFFF
SENTINEL = np.uint64(0x7FF8DEADBEEF0001)  # a NaN pattern no render writes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    neq = bits(got) != bits(want)
    assert not neq.any(), f"{what}: {int(neq.sum())} of {got.size} values differ (first at {int(np.flatnonzero(neq)[0])})"


def tile_order(w, h):
    """Every pixel in the dense render's order: 8x8 tiles row-major, a tile's 64 entries row-major, PAD outside the frame."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    idx = np.arange(tx * ty * 64, dtype=np.int64)
    k, p = idx >> 6, idx & 63
    i, j = (k % tx) * 8 + (p & 7), (k // tx) * 8 + (p >> 3)
    return np.where((i < w) & (j < h), j * w + i, PAD).astype(np.uint32)


def pad64(n):
    return (int(n) + 63) & ~63


def replay(S, Q, n, rel, abs_):
    """The rule of include/rt_amd.h in numpy, elementwise f64 in the same order (numpy does not contract)."""
    m = S / float(n)
    v = (Q - S * m) / float(n - 1)
    e2 = np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2]) / float(n)
    L = ((m[:, 0] + m[:, 1]) + m[:, 2]) / 3.0
    tol = rel * L + abs_
    finite = np.isfinite(S).all(axis=1) & np.isfinite(Q).all(axis=1) & ~np.isnan(v).any(axis=1)
    return finite & (e2 <= tol * tol)


def launches_for(entries, n_samples, budget_bytes, overlap=True):
    """(launches, samples per launch, pipelined?) of one launch_render call (rt_api.cpp): `entries` jobs per sample (the local tiles
    or the list's groups of 64, times 64), 24 bytes each; the chunk is what the sample buffer holds — half of it when a render of
    several launches alternates between two scratch sets.  A chunk of 0: the render is refused."""
    row = pad64(entries) * 24
    chunk = min(budget_bytes // row, (1 << 31) // pad64(entries), n_samples)
    if chunk < 1:
        return 0, 0, False
    half = min((budget_bytes // 2) // row, (1 << 31) // pad64(entries), n_samples)
    pipelined = bool(overlap) and chunk < n_samples and half >= 1
    if pipelined:
        chunk = half
    return -(-n_samples // chunk), chunk, pipelined


def oracle_schedule(rt, oracle, hs, points, seed=3, **oracle_kw):
    """The oracle's running sums and sequential squared sums at each schedule point: {n: (n_pix, 3)} twice.  The sums are rendered
    with accumulate = 1 from point to point, the squares from single-sample renders (q = q + c * c, each product rounded before it is
    added); the sequential sum of those single samples must equal the accumulated snapshot."""
    n_pix = hs.width * hs.height
    snap, snap_q = {}, {}
    run = np.zeros(n_pix * 3)
    s_seq = np.zeros(n_pix * 3)
    q_seq = np.zeros(n_pix * 3)
    prev = 0
    for nk in points:
        oracle.render(hs, rt.render_params(seed=seed, sample_begin=prev, sample_end=nk, accumulate=prev > 0), out=run, **oracle_kw)
        for s in range(prev, nk):
            c = oracle.render(hs, rt.render_params(seed=seed, sample_begin=s, sample_end=s + 1), **oracle_kw)
            s_seq = s_seq + c
            q_seq = q_seq + c * c
        assert_bits(s_seq, run, f"oracle: sequential single samples against the accumulated snapshot at {nk}")
        snap[nk], snap_q[nk] = run.copy().reshape(n_pix, 3), q_seq.copy().reshape(n_pix, 3)
        prev = nk
    return snap, snap_q


def replay_schedule(snap, snap_q, points, rel, abs_):
    """The schedule over the oracle's sums: per pixel the sample count it stops at, the number of batches, and per batch the number of
    pixels still active when it was rendered."""
    n_pix = snap[points[0]].shape[0]
    max_spp = points[-1]
    want_spp = np.zeros(n_pix, dtype=np.int32)
    active = np.ones(n_pix, dtype=bool)
    launches, active_per_batch = 0, []
    for nk in points:
        launches += 1
        active_per_batch.append(int(active.sum()))
        leave = active & (replay(snap[nk], snap_q[nk], nk, rel, abs_) | (nk == max_spp))
        want_spp[leave] = nk
        active &= ~leave
        if not active.any():
            break
    return want_spp, launches, active_per_batch


def check_adaptive_against_oracle(rt, oracle, hs, ds, min_spp, batch, max_spp, rel, abs_, seed=3, min_share=None, **oracle_kw):
    """rt_render_adaptive against the oracle and the numpy replay of the rule: every pixel's spp, its sums and squared sums at the
    point where it stopped (bit for bit), and the result's samples, launches and converged.  min_share: the schedule must not
    degenerate under the ORACLE's sums — at least three schedule points each take that share of the pixels, the last among them."""
    n_pix = hs.width * hs.height
    points = list(range(min_spp, max_spp, batch)) + [max_spp]
    snap, snap_q = oracle_schedule(rt, oracle, hs, points, seed, **oracle_kw)
    want_spp, launches, _ = replay_schedule(snap, snap_q, points, rel, abs_)
    if min_share is not None:
        share = {nk: float((want_spp == nk).mean()) for nk in points}
        assert sum(s >= min_share for s in share.values()) >= 3 and share[max_spp] >= min_share, f"the schedule degenerates: {share}"

    total, spp, sq, res = ds.render_adaptive(rt.render_params(seed=seed, sample_end=max_spp), min_spp=min_spp, batch_spp=batch, rel=rel,
                                             abs=abs_)
    spp = spp.reshape(-1)
    assert (spp == want_spp).all(), f"{int((spp != want_spp).sum())} pixels' spp differ from the replay"
    assert (spp == min_spp).any() and (spp == max_spp).any(), np.unique(spp)
    total, sq = total.reshape(n_pix, 3), sq.reshape(n_pix, 3)
    for nk in points:
        sel = spp == nk
        assert_bits(total[sel], snap[nk][sel], f"sums of the pixels that stopped at {nk}")
        assert_bits(sq[sel], snap_q[nk][sel], f"squared sums of the pixels that stopped at {nk}")
    assert res["samples"] == int(spp.sum())
    assert res["launches"] == launches
    assert res["converged"] == int((spp < max_spp).sum())
    return want_spp
