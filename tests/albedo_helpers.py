"""Shared by the albedo-guided denoise tests (not a test module): the material rule of include/rt_amd.h "albedo scene" in Python, on
a copy of a scene's description that the oracle (or the device) can render, and the normative definition of "albedo-guided denoise"
in numpy, vectorised over pixels with the taps in the stated order.

As in denoise_helpers, every line of the filter is one elementwise f64 operation (numpy neither contracts a * b + c nor replaces a
division by a reciprocal multiply), a tap that is skipped leaves its pixel's sums untouched, and max(a, b) is b > a ? b : a."""
import ctypes as C

import numpy as np

from denoise_helpers import G3, H5, _shifted, display  # noqa: F401  (display: the bytes of a frame of means)

DEFAULTS = dict(iterations=4, sigma=4.0, eps=1e-6, sigma_albedo=0.5, albedo_floor=1e-3)


# ---- the material rule ----
def albedo_rule(rt, desc):
    """(materials, textures): the rule applied to desc's tables, as lists of rt.Material / rt.Texture copies"""
    textures = [rt.Texture.from_buffer_copy(desc.textures[t]) for t in range(desc.n_textures)]
    materials = []

    def solid(r, g, b):
        textures.append(rt.Texture(kind=rt.RT_TEXTURE_SOLID, even=-1, odd=-1, image=-1, perlin=-1, color=rt.Vec3(r, g, b)))
        return len(textures) - 1

    for k in range(desc.n_materials):
        m = desc.materials[k]
        if m.kind in (rt.RT_MATERIAL_LAMBERTIAN, rt.RT_MATERIAL_ISOTROPIC):
            materials.append(rt.Material(kind=rt.RT_MATERIAL_DIFFUSE_LIGHT, texture=m.texture))
        elif m.kind == rt.RT_MATERIAL_METAL:
            materials.append(rt.Material(kind=rt.RT_MATERIAL_DIFFUSE_LIGHT, texture=solid(m.albedo.x, m.albedo.y, m.albedo.z)))
        elif m.kind == rt.RT_MATERIAL_DIELECTRIC:
            materials.append(rt.Material(kind=rt.RT_MATERIAL_DIFFUSE_LIGHT, texture=solid(1.0, 1.0, 1.0)))
        elif m.kind == rt.RT_MATERIAL_DIFFUSE_LIGHT:
            materials.append(rt.Material.from_buffer_copy(m))
        else:
            raise ValueError(f"materials[{k}].kind {m.kind}")
    return materials, textures


def white_camera(rt, camera):
    """the camera the layers above the ABI render an albedo scene with: the beauty camera, background (1, 1, 1)"""
    cam = rt.Camera.from_buffer_copy(camera)
    cam.background = rt.Vec3(1.0, 1.0, 1.0)
    return cam


class AlbedoScene:
    """A scene's description with the rule's materials and textures swapped in (everything else is the original's memory, which it
    keeps alive) and the white-background camera: quacks like rt.HostScene for the oracle and rt.DeviceScene."""

    def __init__(self, rt, host_scene):
        self.original = host_scene
        materials, textures = albedo_rule(rt, host_scene.desc)
        self._materials = (rt.Material * max(1, len(materials)))(*materials)
        self._textures = (rt.Texture * max(1, len(textures)))(*textures)
        d = rt.SceneDesc.from_buffer_copy(host_scene.desc)
        d.materials = self._materials
        d.n_textures, d.textures = len(textures), self._textures
        self.desc = d
        self.camera = white_camera(rt, host_scene.camera)

    width = property(lambda self: self.camera.image_width)
    height = property(lambda self: self.camera.image_height)


def table_bytes(pointer, n):
    """the bytes of the n records a description's table pointer points to"""
    return C.string_at(C.addressof(pointer.contents), n * C.sizeof(pointer._type_)) if n else b""


# ---- the filter ----
def _max(a, b):
    return np.where(b > a, b, a)


def prepare(S, Q, n, A, n_a, albedo_floor):
    """(C0 (h, w, 3), V0 (h, w), valid (h, w), a (h, w, 3), d (h, w, 3)); n: an int or an (h, w) integer array"""
    S, Q, A = (np.asarray(x, dtype=np.float64) for x in (S, Q, A))
    h, w = S.shape[:2]
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (h, w))
    dn = n.astype(np.float64)[:, :, None]
    with np.errstate(all="ignore"):
        m = S / dn
        a = A / float(n_a)
        valid = (n >= 2) & np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2) & np.isfinite(A).all(axis=2)
        d = _max(a, np.float64(albedo_floor))
        I = m / d
        v = (Q - S * m) / (dn - 1.0)
        u = v / (d * d)
        umax = _max(_max(_max(u[:, :, 0], u[:, :, 1]), u[:, :, 2]), 0.0)
        V = umax / dn[:, :, 0]
    return np.where(valid[:, :, None], I, m), np.where(valid, V, -1.0), valid, a, d


def iterate(C, V, valid, a, stride, sigma, eps, sigma_albedo):
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
                aq = _shifted(a, oy, ox, 0.0)
                da = _max(_max(np.abs(a[:, :, 0] - aq[:, :, 0]), np.abs(a[:, :, 1] - aq[:, :, 1])), np.abs(a[:, :, 2] - aq[:, :, 2]))
                y = da / sigma_albedo
                ta = 1.0 - y * y
                ea = np.where(ta > 0.0, ta * ta, 0.0)
                wq = (H5[dy + 2] * H5[dx + 2]) * (e * ea)
                sw = np.where(ok, sw + wq, sw)
                for c in range(3):
                    sc[c] = np.where(ok, sc[c] + wq * _shifted(C[:, :, c], oy, ox, 0.0), sc[c])
                sv = np.where(ok, sv + (wq * wq) * _shifted(V, oy, ox, 0.0), sv)
        Cn = np.stack([np.where(valid, sc[c] / sw, C[:, :, c]) for c in range(3)], axis=2)
        Vn = np.where(valid, sv / (sw * sw), V)
    return Cn, Vn


def denoise_albedo(S, Q, n, A, n_a, iterations=DEFAULTS["iterations"], sigma=DEFAULTS["sigma"], eps=DEFAULTS["eps"],
                   sigma_albedo=DEFAULTS["sigma_albedo"], albedo_floor=DEFAULTS["albedo_floor"]):
    """out, an (h, w, 3) float64 frame: C_K * d for a valid pixel, m for any other"""
    C, V, valid, a, d = prepare(S, Q, n, A, n_a, albedo_floor)
    for k in range(iterations):
        C, V = iterate(C, V, valid, a, 1 << k, sigma, eps, sigma_albedo)
    with np.errstate(all="ignore"):
        return np.where(valid[:, :, None], C * d, C)


def synthetic_albedo(w, h, seed, n_a=4):
    """(A, n_a): sums of n_a made-up albedo samples per pixel — smooth ramps with hard vertical and horizontal edges, a patch of exact
    zeros, a patch below any sensible floor (1e-5), a patch above one (1.75), and a few NaN and +-inf entries."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([0.15 + 0.7 * xx / max(w - 1, 1), 0.8 - 0.6 * yy / max(h - 1, 1), 0.4 + 0.0 * xx], axis=2)
    a[:, w // 2:, :] = a[:, w // 2:, :] * 0.5 + 0.45                          # a hard vertical edge
    a[h // 2:, :, 1] = 0.9 - a[h // 2:, :, 1]                                  # a hard horizontal one in one channel
    a = a + 0.01 * rng.standard_normal((h, w, 3))                              # (anti-aliasing noise)
    qy, qx = max(h // 5, 1), max(w // 7, 1)
    a[0:qy, 0:qx, :] = 0.0
    a[h - qy:h, 0:qx, :] = 1e-5
    a[0:qy, w - qx:w, :] = 1.75
    A = a * float(n_a)
    if w * h >= 15:
        bad = rng.choice(w * h, size=min(5, w * h // 5), replace=False)
        for k, p in enumerate(bad):
            A.reshape(-1, 3)[p, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    return A, n_a
