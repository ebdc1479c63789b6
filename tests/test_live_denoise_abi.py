"""Live denoise's C ABI without a GPU: the four symbols and their Rust declarations, every refusal of rt_render_mean_moments[_device],
rt_denoise_mean_device and rt_denoise_albedo_mean_device (the field named, before the scene handle or a device is touched), struct_size
handled as the sums forms handle it, the command line's refusals, and the numpy restatements of tests/live_denoise_helpers.py — the
Welford fold and the means-form prepare, plain and guided — held to exact rational arithmetic rounded once per operation.

The fold's two properties that (Q - S * m) lacks are checked on the restatement itself: every term d * (c - m') is >= 0 (random, scaled
from 1e-300 to 1e150, and sparse samples), and equal samples give M2 = +0.0 exactly."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import live_denoise_helpers as ldh

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("rt_render_mean_moments_device", "rt_render_mean_moments", "rt_denoise_mean_device", "rt_denoise_albedo_mean_device")


def test_the_symbols_are_exported_declared_and_bound(rt):
    lib = rt.amd_lib()
    header = (ROOT / "include" / "rt_amd.h").read_text()
    text = (ROOT / "INTEGRATION.md").read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(rt.LIB_DIR / "librt_amd.so")], check=True, capture_output=True, text=True).stdout
    for fn in SYMBOLS:
        assert getattr(lib, fn) is not None
        assert fn in rt.RT_AMD_SYMBOLS, fn
        assert f"int {fn}(" in header, fn
        assert f"pub fn {fn}(" in text, fn
        assert re.search(r" T " + fn + r"$", exported, flags=re.M), fn
    for name in ("render_mean_moments", "render_mean_moments_device"):
        assert callable(getattr(rt.DeviceScene, name))
    for name in ("denoise_mean_device", "denoise_mean", "denoise_albedo_mean_device", "denoise_albedo_mean"):
        assert callable(getattr(rt, name))


# ---- the restatements against exact rational arithmetic ----
def _r(x):
    return float(x)  # Fraction -> the nearest double, ties to even: one correctly rounded operation


def _hex(a):
    return [float(x).hex() for x in np.asarray(a).reshape(-1)]


def _exact_fold(samples, m=0.0, m2=0.0, first=0):
    for k, c in enumerate(samples):
        d = _r(Fraction(c) - Fraction(m))
        step = _r(Fraction(d) / (first + k + 1))
        m1 = _r(Fraction(m) + Fraction(step))
        t = _r(Fraction(c) - Fraction(m1))
        p = _r(Fraction(d) * Fraction(t))
        m2 = _r(Fraction(m2) + Fraction(p))
        m = m1
    return m, m2


def test_the_fold_is_the_definition_rounded_once_per_operation():
    rng = np.random.default_rng(3)
    colours = [rng.random((2, 2, 3)) * (10.0 ** rng.integers(-3, 3, size=(2, 2, 3))) for _ in range(6)]
    colours[2][0, 0, :] = colours[1][0, 0, :]  # a repeated sample
    m, q = ldh.fold_moments(colours)
    want = [_exact_fold([float(c.reshape(-1)[v]) for c in colours]) for v in range(12)]
    assert _hex(m) == [w[0].hex() for w in want] and _hex(q) == [w[1].hex() for w in want]
    # the mean is the live route's, and a continuation is the fold of all
    assert _hex(m) == _hex(ldh.live_helpers.fold(colours))
    m3, q3 = ldh.fold_moments(colours[:3])
    m6, q6 = ldh.fold_moments(colours[3:], mean=m3, m2=q3, first=3)
    assert _hex(m6) == _hex(m) and _hex(q6) == _hex(q)
    # M2 is neither Q - S * m nor its value computed another way round: the two agree closely and differ in bits
    v, S, Q = ldh.sums_variance(colours)
    other = Q - S * (S / 6.0)
    assert (q.view(np.uint64) != other.view(np.uint64)).any()
    assert np.allclose(q, other, rtol=1e-9, atol=0.0)
    # the product is rounded before it is added: one sample pair where a fused d * t + M2 would differ
    found = False
    for a, b, c in rng.random((200, 3)):
        m_ab, q_ab = _exact_fold([a, b])
        d = _r(Fraction(c) - Fraction(m_ab))
        m1 = _r(Fraction(m_ab) + Fraction(_r(Fraction(d) / 3)))
        t = _r(Fraction(c) - Fraction(m1))
        fused = _r(Fraction(q_ab) + Fraction(d) * Fraction(t))
        if fused != _exact_fold([a, b, c])[1]:
            found = True
            assert float(ldh.fold_moments([np.array([x]) for x in (a, b, c)])[1][0]).hex() == _exact_fold([a, b, c])[1].hex()
            break
    assert found, "no sample triple tells a contracted update from the definition"


def _max(a, b):
    return b if b > a else a


def test_the_means_form_prepare_is_the_definition_rounded_once_per_operation():
    rng = np.random.default_rng(5)
    h, w, n, floor = 2, 3, 5, 1e-3
    M = rng.random((h, w, 3))
    M2 = rng.random((h, w, 3)) * 0.3
    A = rng.random((h, w, 3))
    M2[0, 1] = (-0.2, -0.1, -0.3)      # every channel negative: V0 = 0
    M2[1, 0, 2] = -0.4                 # one negative channel among positive ones
    A[0, 2] = (0.0, 1e-5, 1.75)        # at, below and above the floor
    M[1, 2, 0] = np.nan                # not valid
    A[1, 1, 1] = np.inf                # not valid in the guided form only
    C0, V0, valid = ldh.prepare_mean(M, M2, n)
    assert valid.tolist() == [[True, True, True], [True, True, False]]
    assert _hex(C0) == _hex(M)
    Cg, Vg, valid_g, a, d = ldh.prepare_albedo_mean(M, M2, n, A, floor)
    assert valid_g.tolist() == [[True, True, True], [True, False, False]]
    assert _hex(a) == _hex(A)
    for y in range(h):
        for x in range(w):
            v = [_r(Fraction(float(M2[y, x, c])) / (n - 1)) for c in range(3)]
            if valid[y, x]:
                assert float(V0[y, x]).hex() == _r(Fraction(_max(_max(_max(v[0], v[1]), v[2]), 0.0)) / n).hex(), (y, x)
            else:
                assert V0[y, x] == -1.0
            if valid_g[y, x]:
                dd = [_max(float(A[y, x, c]), floor) for c in range(3)]
                u = [_r(Fraction(v[c]) / Fraction(_r(Fraction(dd[c]) * Fraction(dd[c])))) for c in range(3)]
                assert float(Vg[y, x]).hex() == _r(Fraction(_max(_max(_max(u[0], u[1]), u[2]), 0.0)) / n).hex(), (y, x)
                assert _hex(Cg[y, x]) == [_r(Fraction(float(M[y, x, c])) / Fraction(dd[c])).hex() for c in range(3)], (y, x)
                assert _hex(d[y, x]) == [float(t).hex() for t in dd]
            else:
                assert Vg[y, x] == -1.0 and _hex(Cg[y, x]) == _hex(M[y, x])
    assert V0[0, 1] == 0.0 and V0[1, 0] > 0.0
    # fewer than two samples: nothing is valid and the output is the input mean, bit for bit — non-finite entries included
    for k in (1, 3):
        assert _hex(ldh.denoise_mean(M, M2, 1, iterations=k)) == _hex(M)
        assert _hex(ldh.denoise_albedo_mean(M, M2, 1, A, iterations=k)) == _hex(M)
    # with the albedo mean 1 everywhere the guided form is the plain one
    ones = np.ones_like(M)
    assert _hex(ldh.denoise_albedo_mean(M, M2, n, ones, iterations=2)) == _hex(ldh.denoise_mean(M, M2, n, iterations=2))
    # and on moments that describe the same samples the means form agrees with the sums form closely, not in bits
    colours = [rng.random((h, w, 3)) for _ in range(n)]
    m, q = ldh.fold_moments(colours)
    _, S, Q = ldh.sums_variance(colours)
    assert np.allclose(ldh.denoise_mean(m, q, n), ldh.denoise_helpers.denoise(S, Q, n), rtol=1e-9)


@pytest.mark.parametrize("kind", ["random", "scaled", "sparse"])
def test_every_term_of_m2_is_at_least_zero(kind):
    rng = np.random.default_rng({"random": 1, "scaled": 2, "sparse": 3}[kind])
    n_pix, n = 4096, 40
    if kind == "random":
        colours = [rng.random(n_pix) for _ in range(n)]
    elif kind == "scaled":
        scale = 10.0 ** rng.uniform(-300.0, 150.0, size=n_pix)
        colours = [rng.random(n_pix) * scale for _ in range(n)]
    else:  # mostly zero, a few bright
        colours = [np.where(rng.random(n_pix) < 0.05, rng.random(n_pix) * 50.0, 0.0) for _ in range(n)]
    terms = []
    m, q = ldh.fold_moments(colours, terms=terms)
    assert len(terms) == n
    prev = np.zeros(n_pix)
    run_q = np.zeros(n_pix)
    for p in terms:
        assert (p >= 0.0).all() and not np.isnan(p).any()
        run_q = run_q + p
        assert (run_q >= prev).all()  # M2 never decreases
        prev = run_q
    assert (q >= 0.0).all() and not np.signbit(q).any()
    # a continuation from any split point has the same property
    terms = []
    m5, q5 = ldh.fold_moments(colours[:5])
    ldh.fold_moments(colours[5:], mean=m5, m2=q5, first=5, terms=terms)
    assert all((p >= 0.0).all() for p in terms)
    # where the sums form goes negative: samples equal to within 1e-15
    near = [1.0 + 1e-15 * rng.standard_normal(n_pix) for _ in range(n)]
    v, _, _ = ldh.sums_variance(near)
    assert (v < 0.0).any(), "Q - S * m stayed non-negative on nearly equal samples: the comparison shows nothing"
    assert (ldh.fold_moments(near)[1] >= 0.0).all()


def test_equal_samples_give_m2_of_plus_zero_exactly():
    rng = np.random.default_rng(7)
    value = np.concatenate([rng.random(500), rng.random(500) * 1e-300, rng.random(500) * 1e150, -rng.random(500), [0.0, -0.0, 1.0 / 3.0, 0.1]])
    for n in (1, 2, 3, 7, 40):
        m, q = ldh.fold_moments([value] * n)
        assert (q.view(np.uint64) == 0).all(), n   # +0.0: not -0.0, not a rounding residue
        assert (m == value).all(), n
    v, _, _ = ldh.sums_variance([value] * 7)
    assert (v != 0.0).any(), "Q - S * m is exactly zero on equal samples too: the comparison shows nothing"


# ---- refusals ----
def _render(rt, *, params=None, camera=True, mean=True, m2=True, rgba8=True, device=False, misalign=False):
    """One call of rt_render_mean_moments (or its device form) with a NULL scene: only argument checks can answer."""
    lib = rt.amd_lib()
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    cam = hs.camera
    p = params if params is not None else rt.render_params(seed=1)
    n = cam.image_width * cam.image_height
    out_mean, out_m2 = (C.c_double * (3 * n))(), (C.c_double * (3 * n))()
    out_rgba = (C.c_uint8 * (4 * n + 4))()
    args = [None, C.byref(cam) if camera else None, C.byref(p) if p is not False else None, C.addressof(out_mean) if mean else None,
            C.addressof(out_m2) if m2 else None, (C.addressof(out_rgba) + (1 if misalign else 0)) if rgba8 else None]
    rc = lib.rt_render_mean_moments_device(*args, None) if device else lib.rt_render_mean_moments(*args)
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("device", [False, True])
def test_every_invalid_render_argument_is_named_before_the_scene_is_looked_at(rt, device):
    cases = [
        (dict(camera=False), "camera"),
        (dict(params=False), "params"),
        (dict(mean=False), "d_mean is null" if device else "mean is null"),
        (dict(m2=False), "d_m2 is null" if device else "m2 is null"),
        (dict(mean=False, m2=False), "d_mean is null" if device else "mean is null"),
        (dict(params=rt.render_params(accumulate=True)), "accumulate"),
        (dict(params=rt.render_params(shard_count=2)), "shard_count"),
        (dict(params=rt.render_params(out_layout=rt.RT_OUT_TILES)), "out_layout"),
        (dict(params=rt.render_params(sample_begin=-1)), "sample_begin"),
        (dict(params=rt.render_params(sample_begin=3, sample_end=3)), "sample_begin, sample_end"),
        (dict(params=rt.render_params(sample_begin=5, sample_end=2)), "sample_begin, sample_end"),
        (dict(params=rt.render_params(sample_begin=8)), "sample_begin, sample_end"),  # sample_end 0: the camera's 8 spp, so [8, 8)
        (dict(m2=False, params=rt.render_params(accumulate=True)), "m2 is null"),     # the pointers come before the parameters
        (dict(), "scene"),             # every other argument is fine: the null scene is what is left
        (dict(rgba8=False), "scene"),  # the display frame is optional
        (dict(params=rt.render_params(sample_begin=7)), "scene"),
    ]
    if device:
        cases.append((dict(misalign=True), "d_rgba8"))
    for kw, field in cases:
        rc, msg = _render(rt, device=device, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg, (kw, msg)
        assert msg.startswith("rt_render_mean_moments_device: " if device else "rt_render_mean_moments: "), (kw, msg)


def _filter(rt, guided, *, w=6, h=4, m=True, q=True, a=True, samples=8, params=None, out=True, rgba=True, ws=True, alias=None, misalign=False,
            ws_misalign=False):
    """One call of rt_denoise_mean_device / rt_denoise_albedo_mean_device on HOST buffers: only argument checks can answer (the first
    thing past them asks the HIP runtime which device owns d_mean_out, and host memory has none)."""
    lib = rt.amd_lib()
    n = min(w * h, 4096) if w > 0 and h > 0 else 1   # (a frame the size check refuses is never touched: no need to allocate it)
    M, Q, A, O = ((C.c_double * (3 * n))() for _ in range(4))
    B = (C.c_uint8 * (4 * n + 4))()
    W = (C.c_uint8 * (96 * n + 32))()
    ws_ptr = (C.addressof(W) + 15) // 16 * 16 + (8 if ws_misalign else 0)
    out_ptr = C.addressof(O)
    if alias == "mean":
        out_ptr = C.addressof(M) + 8 * (3 * n - 1)   # the last double of M
    elif alias == "m2":
        out_ptr = C.addressof(Q)
    elif alias == "albedo":
        out_ptr = C.addressof(A) - 8 * (3 * n - 1)   # ends in A's first double
    head = [w, h, C.addressof(M) if m else None, C.addressof(Q) if q else None, samples]
    tail = [C.byref(params) if params is not None else None, out_ptr if out else None, (C.addressof(B) + (1 if misalign else 0)) if rgba else None,
            ws_ptr if ws else None, None]
    if guided:
        rc = lib.rt_denoise_albedo_mean_device(*head, C.addressof(A) if a else None, *tail)
    else:
        rc = lib.rt_denoise_mean_device(*head, *tail)
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("guided", [False, True])
def test_every_invalid_filter_argument_is_named_without_a_device(rt, guided):
    P = rt.DenoiseAlbedoParams if guided else rt.DenoiseParams
    make = rt.denoise_albedo_params if guided else rt.denoise_params
    who = "rt_denoise_albedo_mean_device: " if guided else "rt_denoise_mean_device: "
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(m=False), "d_mean is null"),
        (dict(q=False), "d_m2 is null"),
        (dict(out=False), "d_mean_out is null"),
        (dict(ws=False), "d_workspace is null"),
        (dict(w=0), "width"), (dict(h=-3), "height"), (dict(w=1 << 14, h=1 << 13), "2^27"),
        (dict(samples=0), "samples"), (dict(samples=-4), "samples"),
        (dict(params=P(struct_size=12, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=48, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        (dict(params=P(struct_size=0)), "struct_size"),
        (dict(params=make(iterations=0)), "iterations"), (dict(params=make(iterations=7)), "iterations"),
        (dict(params=make(sigma=0.0)), "sigma"), (dict(params=make(sigma=nan)), "sigma"), (dict(params=make(sigma=inf)), "sigma"),
        (dict(params=make(eps=0.0)), "eps"), (dict(params=make(eps=nan)), "eps"),
        (dict(alias="mean"), "d_mean_out must not overlap"), (dict(alias="m2"), "d_mean_out must not overlap"),
        (dict(misalign=True), "d_rgba8"),
        (dict(ws_misalign=True), "d_workspace"),
        # the documented order: a pointer before the frame's size is past, the sample count before the params, the params in field order
        (dict(q=False, samples=0), "d_m2 is null"),
        (dict(samples=0, params=make(iterations=0)), "samples"),
        (dict(params=make(iterations=0, sigma=0.0, eps=0.0)), "iterations"),
        (dict(params=make(sigma=0.0, eps=0.0), alias="m2"), "sigma"),
        (dict(alias="m2", misalign=True), "d_mean_out must not overlap"),
    ]
    if guided:
        cases += [
            (dict(a=False), "d_albedo_mean is null"),
            (dict(alias="albedo"), "d_mean_out must not overlap"),
            (dict(params=make(sigma_albedo=0.0)), "sigma_albedo"), (dict(params=make(sigma_albedo=nan)), "sigma_albedo"),
            (dict(params=make(albedo_floor=0.0)), "albedo_floor"), (dict(params=make(albedo_floor=inf)), "albedo_floor"),
            (dict(params=P(struct_size=44, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"),
        ]
    else:
        cases.append((dict(params=P(struct_size=32, iterations=4, sigma=4.0, eps=1e-6)), "struct_size"))
    for kw, field in cases:
        rc, msg = _filter(rt, guided, **kw)
        assert rc == -1, (kw, rc, msg)
        assert field in msg and msg.startswith(who), (kw, msg)
        assert "d_sum" not in msg and "d_albedo_sum" not in msg, (kw, msg)   # the inputs are named as THIS entry point names them
    # what is optional, or fine, gets past every check: what answers then is the look-up of the device that owns a HOST pointer.
    # samples = 1 is fine (the output is the input mean), and struct_size is handled as in the sums forms: a shorter struct of an
    # older caller is accepted, and the fields it lacks are the defaults, not the bytes behind it
    fine = [dict(), dict(rgba=False), dict(samples=1), dict(samples=2), dict(params=make(iterations=6)),
            dict(params=make(iterations=1, sigma=0.5, eps=1e-12)), dict(params=P(struct_size=8, iterations=2)),
            dict(params=P(struct_size=16, iterations=2, sigma=1.0)), dict(params=P(struct_size=16, iterations=2, sigma=1.0, eps=0.0))]
    if guided:
        fine += [dict(params=P(struct_size=24, iterations=2, sigma=1.0, eps=1e-6, sigma_albedo=0.0, albedo_floor=0.0)),
                 dict(params=P(struct_size=32, iterations=2, sigma=1.0, eps=1e-6, sigma_albedo=0.25, albedo_floor=-1.0))]
    for kw in fine:
        rc, msg = _filter(rt, guided, **kw)
        assert rc != 0 and "not a device pointer" in msg and msg.startswith(who), (kw, rc, msg)


def test_the_python_wrappers_check_their_frames(rt):
    hs = rt.HostScene(6, width=16, spp=8, depth=4)
    ds = object.__new__(rt.DeviceScene)   # no handle: the wrapper's own checks come first
    ds.host_scene, ds._handle = hs, None
    with pytest.raises(rt.RtError, match="sample_begin"):
        ds.render_mean_moments(rt.render_params(sample_begin=2, sample_end=4))
    with pytest.raises(rt.RtError, match="m2"):
        ds.render_mean_moments(rt.render_params(sample_begin=2, sample_end=4), mean=np.zeros((hs.height, hs.width, 3)))
    with pytest.raises(rt.RtError, match="mean"):
        ds.render_mean_moments(rt.render_params(sample_end=4), mean=np.zeros((3, 3, 3)), m2=np.zeros((hs.height, hs.width, 3)))
    with pytest.raises(rt.RtError, match="one shape"):
        rt.denoise_mean(np.zeros((4, 6, 3)), np.zeros((4, 5, 3)), 4)
    with pytest.raises(rt.RtError, match="one shape"):
        rt.denoise_albedo_mean(np.zeros((4, 6, 3)), np.zeros((4, 6, 3)), 4, np.zeros((4, 6)))
    with pytest.raises(TypeError):
        rt.denoise_mean(np.zeros((4, 6, 3)), np.zeros((4, 6, 3)), 4, sigma_albedo=0.3)


def test_rtrace_refuses_the_new_flags_without_live_and_a_knob_without_its_flag(rt, tmp_path):
    exe = rt.LIB_DIR / "rtrace"
    assert exe.exists(), "run build() first"
    base = ["-s", "6", "--width", "16", "--spp", "4", "--depth", "4", "-o", str(tmp_path / "x")]
    cases = [
        (["--live-denoise"], "--live"), (["--live-denoise-albedo"], "--live"),
        (["--live-denoise", "--denoise-iters", "2"], "--live"),
        (["--live", "--denoise-iters", "3"], "--live-denoise"), (["-l", "--denoise-sigma", "2"], "--live-denoise"),
        (["--live", "--denoise-albedo-sigma", "0.3"], "--live-denoise-albedo"),
        (["--live", "--live-denoise", "--denoise-albedo-sigma", "0.3"], "--live-denoise-albedo"),
        # every existing refusal stays: the batch filters cannot take the live route
        (["--live", "--denoise"], "--denoise"), (["--live", "--live-denoise", "--denoise"], "--denoise"),
        (["--live", "--denoise-albedo"], "--denoise"),
        (["--live", "--live-denoise", "--gpus", "2"], "--live"), (["--live", "--live-denoise", "--adaptive", "0.05"], "--live"),
    ]
    for extra, word in cases:
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (extra, r.returncode, r.stderr)
        assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (extra, r.stderr)
    for extra in (["--live", "--live-denoise", "--denoise-iters", "7"], ["--live", "--live-denoise", "--denoise-sigma", "0"],
                  ["--live", "--live-denoise-albedo", "--denoise-albedo-sigma", "0"]):
        r = subprocess.run([str(exe), *base, *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--denoise" in r.stderr, (extra, r.returncode, r.stderr)
    r = subprocess.run([str(exe), "-s", "6", "--live", "--live-denoise"], capture_output=True, text=True, timeout=60)   # no -o
    assert r.returncode == 2 and "--output" in r.stderr, r.stderr
    assert not list(tmp_path.iterdir())
    usage = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60).stderr
    assert "--live-denoise " in usage and "--live-denoise-albedo" in usage
