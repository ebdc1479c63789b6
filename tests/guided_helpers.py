"""Shared by the edge-guided denoise tests (not a test module): the surface-ID rule of include/rt_amd.h "surface-ID scene" in Python,
on a copy of a scene's description that the oracle (or the device) can render, and the normative definition of "edge-guided denoise"
in numpy, vectorised over pixels with the taps in the stated order.

As in denoise_helpers and albedo_helpers, every line of the filter is one elementwise f64 operation (numpy neither contracts
a * b + c nor replaces a division by a reciprocal multiply), a tap that is skipped leaves its pixel's sums untouched, and max(a, b) is
b > a ? b : a.  With A None the filter is the plain one with the edge stop; otherwise the albedo-guided one with it."""
import numpy as np

from albedo_helpers import table_bytes  # noqa: F401  (the bytes of a description's table)
from denoise_helpers import G3, H5, _shifted, display  # noqa: F401  (display: the bytes of a frame of means)

COLOURS = 26
DEFAULTS = dict(iterations=4, sigma=4.0, eps=1e-6, sigma_albedo=0.5, albedo_floor=1e-3, sigma_edge=0.5)


# ---- the surface-ID rule ----
def palette(q):
    """palette entry q, 1..26"""
    assert 1 <= q <= COLOURS
    return (0.5 * (q % 3), 0.5 * ((q // 3) % 3), 0.5 * (q // 9))


def id_rule(rt, desc):
    """(spheres, quads, media, materials, textures): the rule applied to desc's tables, as lists of ctypes copies"""
    textures = [rt.Texture(kind=rt.RT_TEXTURE_SOLID, even=-1, odd=-1, image=-1, perlin=-1, color=rt.Vec3(*palette(i + 1))) for i in range(COLOURS)]
    materials = [rt.Material(kind=rt.RT_MATERIAL_DIFFUSE_LIGHT, texture=i) for i in range(COLOURS)]
    k = 0
    spheres, quads, media = [], [], []
    for i in range(desc.n_spheres):
        s = rt.Sphere.from_buffer_copy(desc.spheres[i])
        s.material = k % COLOURS
        spheres.append(s)
        k += 1
    for i in range(desc.n_quads):
        q = rt.Quad.from_buffer_copy(desc.quads[i])
        q.material = k % COLOURS
        quads.append(q)
        k += 1
    for i in range(desc.n_media):
        m = rt.ConstantMedium.from_buffer_copy(desc.media[i])
        m.phase_material = k % COLOURS
        media.append(m)
        k += 1
    return spheres, quads, media, materials, textures


def black_camera(rt, camera):
    """the camera the layers above the ABI render a surface-ID scene with: the beauty camera, background (0, 0, 0)"""
    cam = rt.Camera.from_buffer_copy(camera)
    cam.background = rt.Vec3(0.0, 0.0, 0.0)
    return cam


class SurfaceIdScene:
    """A scene's description with the rule's five tables and two counts swapped in (everything else is the original's memory, which
    it keeps alive) and the black-background camera: quacks like rt.HostScene for the oracle and rt.DeviceScene."""

    def __init__(self, rt, host_scene):
        self.original = host_scene
        spheres, quads, media, materials, textures = id_rule(rt, host_scene.desc)
        self._spheres = (rt.Sphere * max(1, len(spheres)))(*spheres)
        self._quads = (rt.Quad * max(1, len(quads)))(*quads)
        self._media = (rt.ConstantMedium * max(1, len(media)))(*media)
        self._materials = (rt.Material * COLOURS)(*materials)
        self._textures = (rt.Texture * COLOURS)(*textures)
        d = rt.SceneDesc.from_buffer_copy(host_scene.desc)
        d.spheres, d.quads, d.media = self._spheres, self._quads, self._media
        d.n_materials, d.materials = COLOURS, self._materials
        d.n_textures, d.textures = COLOURS, self._textures
        self.desc = d
        self.camera = black_camera(rt, host_scene.camera)

    width = property(lambda self: self.camera.image_width)
    height = property(lambda self: self.camera.image_height)


# ---- the filter ----
def _max(a, b):
    return np.where(b > a, b, a)


def prepare(S, Q, n, E, n_e, A=None, n_a=0, albedo_floor=DEFAULTS["albedo_floor"]):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w), g (h, w, 3), a, d) — a, d (h, w, 3) or None without an albedo frame;
    n: an int or an (h, w) integer array"""
    S, Q, E = (np.asarray(x, dtype=np.float64) for x in (S, Q, E))
    h, w = S.shape[:2]
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (h, w))
    dn = n.astype(np.float64)[:, :, None]
    with np.errstate(all="ignore"):
        m = S / dn
        g = E / float(n_e)
        valid = (n >= 2) & np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2) & np.isfinite(E).all(axis=2)
        v = (Q - S * m) / (dn - 1.0)
        if A is None:
            a = d = None
            C0, u = m, v
        else:
            A = np.asarray(A, dtype=np.float64)
            a = A / float(n_a)
            valid = valid & np.isfinite(A).all(axis=2)
            d = _max(a, np.float64(albedo_floor))
            C0 = m / d
            u = v / (d * d)
        umax = _max(_max(_max(u[:, :, 0], u[:, :, 1]), u[:, :, 2]), 0.0)
        V = umax / dn[:, :, 0]
    return np.where(valid[:, :, None], C0, m), np.where(valid, V, -1.0), valid, g, a, d


def _stop(x, xq, sigma):
    dd = _max(_max(np.abs(x[:, :, 0] - xq[:, :, 0]), np.abs(x[:, :, 1] - xq[:, :, 1])), np.abs(x[:, :, 2] - xq[:, :, 2]))
    z = dd / sigma
    t = 1.0 - z * z
    return np.where(t > 0.0, t * t, 0.0)


def iterate(C, V, valid, g, a, stride, sigma, eps, sigma_albedo, sigma_edge):
    h, w = V.shape
    with np.errstate(all="ignore"):
        L = ((C[:, :, 0] + C[:, :, 1]) + C[:, :, 2]) / 3.0
        gs, ws = np.zeros((h, w)), np.zeros((h, w))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = _shifted(valid, dy, dx, False)
                k = G3[dy + 1] * G3[dx + 1]
                gs = np.where(ok, gs + k * _shifted(V, dy, dx, 0.0), gs)
                ws = np.where(ok, ws + k, ws)
        G = gs / ws
        sd = np.sqrt(G)
        den = sigma * sd + eps
        sw, sv = np.zeros((h, w)), np.zeros((h, w))
        sc = [np.zeros((h, w)) for _ in range(3)]
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                oy, ox = dy * stride, dx * stride
                ok = _shifted(valid, oy, ox, False)
                x = np.abs(L - _shifted(L, oy, ox, 0.0)) / den
                t = 1.0 - x * x
                e = np.where(t > 0.0, t * t, 0.0)
                if a is not None:
                    e = e * _stop(a, _shifted(a, oy, ox, 0.0), sigma_albedo)
                e = e * _stop(g, _shifted(g, oy, ox, 0.0), sigma_edge)
                wq = (H5[dy + 2] * H5[dx + 2]) * e
                sw = np.where(ok, sw + wq, sw)
                for c in range(3):
                    sc[c] = np.where(ok, sc[c] + wq * _shifted(C[:, :, c], oy, ox, 0.0), sc[c])
                sv = np.where(ok, sv + (wq * wq) * _shifted(V, oy, ox, 0.0), sv)
        Cn = np.stack([np.where(valid, sc[c] / sw, C[:, :, c]) for c in range(3)], axis=2)
        Vn = np.where(valid, sv / (sw * sw), V)
    return Cn, Vn


def denoise_guided(S, Q, n, E, n_e, A=None, n_a=0, iterations=DEFAULTS["iterations"], sigma=DEFAULTS["sigma"], eps=DEFAULTS["eps"],
                   sigma_albedo=DEFAULTS["sigma_albedo"], albedo_floor=DEFAULTS["albedo_floor"], sigma_edge=DEFAULTS["sigma_edge"]):
    """out, an (h, w, 3) float64 frame: C_K (with an albedo frame: C_K * d) for a valid pixel, m for any other"""
    C, V, valid, g, a, d = prepare(S, Q, n, E, n_e, A, n_a, albedo_floor)
    for k in range(iterations):
        C, V = iterate(C, V, valid, g, a, 1 << k, sigma, eps, sigma_albedo, sigma_edge)
    if A is None:
        return C
    with np.errstate(all="ignore"):
        return np.where(valid[:, :, None], C * d, C)


def synthetic_edges(w, h, seed, n_e=4):
    """(E, n_e): sums of n_e made-up samples of a surface-ID frame per pixel — blocks of palette colours a few pixels wide (some
    neighbours 0.5 apart in one channel only, some further), a strip of background black, anti-aliased block borders (means between
    two palette colours, so 0 < eg < 1 happens), and a few NaN and +-inf entries."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ids = ((xx // 5) + 3 * (yy // 4)) % COLOURS + 1
    g = np.stack([0.5 * (ids % 3), 0.5 * ((ids // 3) % 3), 0.5 * (ids // 9)], axis=2).astype(np.float64)
    g[:, w - max(w // 9, 1):, :] = 0.0
    border = (xx % 5 == 0) & (xx > 0)
    left = np.roll(g, 1, axis=1)
    mix = rng.integers(1, n_e, size=(h, w)).astype(np.float64) / n_e          # k / n_e of the samples landed on the left surface
    g = np.where(border[:, :, None], mix[:, :, None] * left + (1.0 - mix[:, :, None]) * g, g)
    E = g * float(n_e)
    if w * h >= 15:
        bad = rng.choice(w * h, size=min(4, w * h // 5), replace=False)
        for k, p in enumerate(bad):
            E.reshape(-1, 3)[p, (k + 1) % 3] = (np.inf, np.nan, -np.inf)[k % 3]
    return E, n_e
