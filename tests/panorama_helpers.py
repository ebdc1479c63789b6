"""Panoramas (include/rt_amd.h "panoramas") restated in numpy, whose elementwise float64 operations are IEEE and never contracted: the
cube-face cameras, the resampler, and the inputs the CPU and GPU tests share."""
import numpy as np

# forward n, up u, right r = n x u per face, as (axis, sign)
AXES = (((0, 1), (1, 1), (2, 1)), ((0, -1), (1, 1), (2, -1)), ((1, 1), (2, 1), (0, 1)),
        ((1, -1), (2, -1), (0, 1)), ((2, 1), (1, 1), (0, -1)), ((2, -1), (1, 1), (0, 1)))
SIZES = ((1, 1), (63, 1), (65, 3), (257, 255))          # (W, H)
FACES = ((2, 0), (3, 1), (5, 2), (16, 1))               # (F, g)
CENTER = (0.1, -2.3, 7.7)                                # no coordinate is dyadic


def cameras_ref(center, F, g):
    """the six cameras' centre, pixel00_loc, pixel_delta_u and pixel_delta_v, each operation rounded on its own"""
    inner = np.float64(F - 2 * g)
    delta = np.float64(2.0) / inner
    hh = np.float64(F) / inner
    e = np.float64(0.5) * delta - hh
    c = np.asarray(center, dtype=np.float64)
    out = []
    for (na, ns), (ua, us), (ra, rs) in AXES:
        t, du, dv = np.zeros(3), np.zeros(3), np.zeros(3)
        t[na] = ns
        t[ra] = e if rs > 0 else -e
        t[ua] = -e if us > 0 else e
        du[ra] = delta if rs > 0 else -delta
        dv[ua] = -delta if us > 0 else delta
        out.append(dict(center=c.copy(), pixel00_loc=c + t, pixel_delta_u=du, pixel_delta_v=dv))
    return out


def vec(v):
    return np.array([v.x, v.y, v.z], dtype=np.float64)


def directions(tables, W, H):
    """(dx, dy, dz), each (H, W), of the output pixels"""
    sl, cl = tables[0:2 * W:2][None, :], tables[1:2 * W:2][None, :]
    sp, cp = tables[2 * W::2][:, None], tables[2 * W + 1::2][:, None]
    return cp * sl, sp + np.zeros_like(sl), -(cp * cl)


def face_map(tables, W, H):
    """(face, m, d.r, d.u) per output pixel, by the header's rule"""
    dx, dy, dz = directions(tables, W, H)
    ax, ay, az = np.abs(dx), np.abs(dy), np.abs(dz)
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    face = np.where(isx, np.where(dx > 0, 0, 1), np.where(isy, np.where(dy > 0, 2, 3), np.where(dz > 0, 4, 5)))
    m = np.where(isx, ax, np.where(isy, ay, az))
    da = np.choose(face, [dz, -dz, dx, dx, -dx, dx])
    db = np.choose(face, [dy, dy, dz, -dz, dy, dy])
    return face, m, da, db


def taps(tables, W, H, F, g):
    """(face, x0, y0, fx, fy) per output pixel"""
    face, m, da, db = face_map(tables, W, H)
    a, b = da / m, db / m
    s = np.float64(F - 2 * g) * 0.5
    c = np.float64(F) * 0.5 - 0.5
    x, y = a * s + c, c - b * s
    x0 = np.clip(np.floor(x).astype(np.int64), 0, F - 2)
    y0 = np.clip(np.floor(y).astype(np.int64), 0, F - 2)
    fx = np.minimum(np.maximum(x - x0.astype(np.float64), 0.0), 1.0)
    fy = np.minimum(np.maximum(y - y0.astype(np.float64), 0.0), 1.0)
    return face, x0, y0, fx, fy


def resample_ref(W, H, tables, faces, g, spp):
    """the (H, W, 3) frame of means the header defines, from (6, F, F, 3) faces"""
    F = faces.shape[1]
    face, x0, y0, fx, fy = taps(tables, W, H, F, g)
    T = faces * (np.float64(1.0) / np.float64(spp))
    with np.errstate(invalid="ignore"):
        T00, T10 = T[face, y0, x0], T[face, y0, x0 + 1]
        T01, T11 = T[face, y0 + 1, x0], T[face, y0 + 1, x0 + 1]
        fx, fy = fx[..., None], fy[..., None]
        top = T00 + (T10 - T00) * fx
        bot = T01 + (T11 - T01) * fx
        return top + (bot - top) * fy


def tapped(tables, W, H, F, g):
    """(H, W, 6, F, F) booleans: the texels among every output pixel's four taps"""
    face, x0, y0, _, _ = taps(tables, W, H, F, g)
    hit = np.zeros((H, W, 6, F, F), dtype=bool)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for dy in (0, 1):
        for dx in (0, 1):
            hit[jj, ii, face, y0 + dy, x0 + dx] = True
    return hit


def random_faces(F, seed, spp):
    rng = np.random.default_rng(seed)
    faces = rng.random((6, F, F, 3)) * 4.0 * spp
    faces.setflags(write=False)
    return faces


def direction_faces(F, g):
    """texel (i, j) of face f holds its own direction under the cameras of the header, divided by its forward component's magnitude"""
    cams = cameras_ref((0.0, 0.0, 0.0), F, g)
    faces = np.zeros((6, F, F, 3))
    i = np.arange(F, dtype=np.float64)
    for f, cam in enumerate(cams):
        d = cam["pixel00_loc"][None, None, :] + i[None, :, None] * cam["pixel_delta_u"][None, None, :] + i[:, None, None] * cam["pixel_delta_v"][None, None, :]
        faces[f] = d / np.abs(d[..., AXES[f][0][0]])[..., None]
    return faces


def own_direction(tables, W, H):
    """d / m per output pixel, (H, W, 3)"""
    dx, dy, dz = directions(tables, W, H)
    d = np.stack([dx, dy, dz], axis=-1)
    return d / np.max(np.abs(d), axis=-1, keepdims=True)


def tie_tables():
    """Hand-made tables of a 12 x 3 frame whose directions tie exactly: the rows have (sp, cp) = (1, 1), (0, 1) and (-1, 1); the columns'
    (sl, cl) give (dx, dz) = (sl, -cl).  Returns (tables, W, H, the face the header prescribes per pixel)."""
    cols = [(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0),      # |dx| = |dz| (and, in row 0, = |dy|): X wins
            (0.5, 1.0), (0.5, -1.0),                                 # row 0: |dy| = |dz| > |dx|: Y over Z; row 1: Z
            (0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0),      # dx a zero of either sign: row 0 |dy| = |dz|: Y; row 1: Z
            (1.0, 0.0), (-1.0, -0.0)]                                # dz a zero of either sign: |dx| = |dy| in row 0: X
    rows = [(1.0, 1.0), (0.0, 1.0), (-1.0, 1.0)]
    W, H = len(cols), len(rows)
    t = np.array([v for c in cols for v in c] + [v for r in rows for v in r], dtype=np.float64)
    want = np.array([[0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 0, 1],
                     [0, 0, 1, 1, 5, 4, 5, 5, 4, 4, 0, 1],
                     [0, 0, 1, 1, 3, 3, 3, 3, 3, 3, 0, 1]])
    return t, W, H, want


def index_faces(F):
    faces = np.zeros((6, F, F, 3))
    faces += np.arange(6, dtype=np.float64)[:, None, None, None]
    return faces


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
