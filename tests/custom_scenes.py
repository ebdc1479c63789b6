"""Hand-made rt_scene_desc graphs for cases the reference's nine scenes never produce: primitives hit at exactly
the same t (coincident copies, overlapping coplanar quads), single-primitive worlds, empty frames.

A CustomScene quacks like rt.HostScene (desc, camera, width, height) for rt.DeviceScene and the oracle."""
from __future__ import annotations

import ctypes as C
import importlib
import math

import numpy as np

rt = importlib.import_module("rust-tracing_amd")


def _v(x, y, z):
    return rt.Vec3(float(x), float(y), float(z))


class CustomScene:
    def __init__(self, camera_from: "rt.HostScene", spp=4, depth=6, background=None):
        self.spheres, self.quads, self.lists, self.items = [], [], [], []
        self.translates, self.rotates, self.materials, self.textures = [], [], [], []
        self.media, self.perlins, self.images = [], [], []
        self.camera = rt.Camera.from_buffer_copy(camera_from.camera)
        self.camera.samples_per_pixel = spp
        self.camera.max_depth = depth
        if background is not None:
            self.camera.background = _v(*background)
        self.desc = None

    width = property(lambda self: self.camera.image_width)
    height = property(lambda self: self.camera.image_height)

    # ---- materials ----
    def solid(self, r, g, b):
        self.textures.append(rt.Texture(kind=rt.RT_TEXTURE_SOLID, even=-1, odd=-1, image=-1, perlin=-1, color=_v(r, g, b)))
        return len(self.textures) - 1

    # ---- textures other than a solid colour: each returns a texture index ----
    def add_perlin(self, table):
        self.perlins.append(rt.Perlin.from_buffer_copy(table))
        return len(self.perlins) - 1

    def add_image(self, rgb):
        """rgb: an (h, w, 3) uint8 array, row-major as rt_image has it"""
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 3 and a.shape[0] > 0 and a.shape[1] > 0
        self.images.append(a)
        return len(self.images) - 1

    def checker(self, scale, even_tex, odd_tex):
        # CheckerTexture::new (src/texture.rs): inv_scale = 1.0 / scale
        self.textures.append(rt.Texture(kind=rt.RT_TEXTURE_CHECKER, even=even_tex, odd=odd_tex, image=-1, perlin=-1, inv_scale=1.0 / scale))
        return len(self.textures) - 1

    def noise(self, scale, perlin):
        self.textures.append(rt.Texture(kind=rt.RT_TEXTURE_NOISE, even=-1, odd=-1, image=-1, perlin=perlin, scale=scale))
        return len(self.textures) - 1

    def image(self, index):
        self.textures.append(rt.Texture(kind=rt.RT_TEXTURE_IMAGE, even=-1, odd=-1, image=index, perlin=-1))
        return len(self.textures) - 1

    def lambertian_tex(self, t):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_LAMBERTIAN, texture=t))
        return len(self.materials) - 1

    def light_tex(self, t):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_DIFFUSE_LIGHT, texture=t))
        return len(self.materials) - 1

    def isotropic_tex(self, t):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_ISOTROPIC, texture=t))
        return len(self.materials) - 1

    def lambertian(self, r, g, b):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_LAMBERTIAN, texture=self.solid(r, g, b)))
        return len(self.materials) - 1

    def light(self, r, g, b):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_DIFFUSE_LIGHT, texture=self.solid(r, g, b)))
        return len(self.materials) - 1

    def metal(self, r, g, b, fuzz):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_METAL, texture=-1, albedo=_v(r, g, b), fuzz=fuzz))
        return len(self.materials) - 1

    def isotropic(self, r, g, b):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_ISOTROPIC, texture=self.solid(r, g, b)))
        return len(self.materials) - 1

    def dielectric(self, ir):
        self.materials.append(rt.Material(kind=rt.RT_MATERIAL_DIELECTRIC, texture=-1, ir=ir))
        return len(self.materials) - 1

    # ---- hittables: each returns an rt.Ref ----
    def sphere(self, center, radius, material, moving_to=None):
        if moving_to is None:
            self.spheres.append(rt.Sphere(center=_v(*center), radius=radius, center_vec=_v(0, 0, 0), is_moving=0, material=material))
        else:  # Sphere::with_target (src/sphere.rs): center_vec = target - center
            vec = tuple(float(t) - float(c) for t, c in zip(moving_to, center))
            self.spheres.append(rt.Sphere(center=_v(*center), radius=radius, center_vec=_v(*vec), is_moving=1, material=material))
        return rt.Ref(rt.RT_HITTABLE_SPHERE, len(self.spheres) - 1)

    def quad(self, q, u, v, material):
        # Quad::new (src/quad.rs:23-43), in Python floats = f64, same operation order as the host mirror
        n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
        rl = 1.0 / math.sqrt(n2)
        normal = (n[0] * rl, n[1] * rl, n[2] * rl)
        d = normal[0] * q[0] + normal[1] * q[1] + normal[2] * q[2]
        w = (n[0] / n2, n[1] / n2, n[2] / n2)
        self.quads.append(rt.Quad(q=_v(*q), u=_v(*u), v=_v(*v), w=_v(*w), normal=_v(*normal), d=d, material=material))
        return rt.Ref(rt.RT_HITTABLE_QUAD, len(self.quads) - 1)

    def list(self, refs):
        first = len(self.items)
        self.items.extend(refs)
        self.lists.append(rt.List(first, len(refs)))
        return rt.Ref(rt.RT_HITTABLE_LIST, len(self.lists) - 1)

    def translate(self, ref, offset):
        self.translates.append(rt.Translate(object=ref, offset=_v(*offset)))
        return rt.Ref(rt.RT_HITTABLE_TRANSLATE, len(self.translates) - 1)

    def rotate_y(self, ref, degrees):
        th = math.radians(degrees)
        self.rotates.append(rt.RotateY(object=ref, sin_theta=math.sin(th), cos_theta=math.cos(th)))
        return rt.Ref(rt.RT_HITTABLE_ROTATE_Y, len(self.rotates) - 1)

    def medium(self, boundary, density, r=None, g=None, b=None, texture=None):
        # ConstantMedium::new (src/constant_medium.rs:21-30): neg_inv_density = -1 / density, phase = Isotropic(colour or texture)
        phase = self.isotropic(r, g, b) if texture is None else self.isotropic_tex(texture)
        self.media.append(rt.ConstantMedium(boundary=boundary, neg_inv_density=-1.0 / density, phase_material=phase))
        return rt.Ref(rt.RT_HITTABLE_CONSTANT_MEDIUM, len(self.media) - 1)

    def finish(self, world: "rt.Ref"):
        def arr(kind, values):
            a = (kind * max(1, len(values)))(*values)
            return a

        self._keep = dict(spheres=arr(rt.Sphere, self.spheres), quads=arr(rt.Quad, self.quads), lists=arr(rt.List, self.lists),
                          items=arr(rt.Ref, self.items), translates=arr(rt.Translate, self.translates),
                          rotates=arr(rt.RotateY, self.rotates), media=arr(rt.ConstantMedium, self.media),
                          materials=arr(rt.Material, self.materials),
                          textures=arr(rt.Texture, self.textures))
        k = self._keep
        d = rt.SceneDesc()
        d.abi_version = rt.RT_ABI_VERSION
        d.world = world
        d.n_spheres, d.spheres = len(self.spheres), k["spheres"]
        d.n_quads, d.quads = len(self.quads), k["quads"]
        d.n_lists, d.lists = len(self.lists), k["lists"]
        d.n_list_items, d.list_items = len(self.items), k["items"]
        d.n_translates, d.translates = len(self.translates), k["translates"]
        d.n_rotates, d.rotates = len(self.rotates), k["rotates"]
        d.n_media, d.media = len(self.media), k["media"]
        d.n_materials, d.materials = len(self.materials), k["materials"]
        d.n_textures, d.textures = len(self.textures), k["textures"]
        if self.perlins:
            k["perlins"] = arr(rt.Perlin, self.perlins)
            d.n_perlins, d.perlins = len(self.perlins), k["perlins"]
        if self.images:
            k["pixels"] = list(self.images)  # the numpy buffers the records point into
            k["images"] = arr(rt.Image, [rt.Image(width=a.shape[1], height=a.shape[0], rgb=a.ctypes.data_as(C.POINTER(C.c_uint8)))
                                         for a in k["pixels"]])
            d.n_images, d.images = len(self.images), k["images"]
        self.desc = d
        return self


# ---- inputs of the textured scenes: made here from fixed seeds, nothing is read from a file ----
_R3 = 1.0 / math.sqrt(3.0)
# where a moving sphere goes, in radii of its own: along both directions of every axis, then along the eight diagonals
MOTIONS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + \
          [(sx * _R3, sy * _R3, sz * _R3) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
IMAGE_SIZES = [(13, 5), (1, 1), (8, 8), (1, 9), (17, 1)]  # (width, height): neither a multiple of the 8x8 texel tile, one tile, one texel wide / high
_perlin_a = []


def random_image(k, width, height, zero_half=False):
    """an (height, width, 3) uint8 image of generator k; zero_half: its upper rows are all zero (texels of exactly (0, 0, 0)) and its
    last texel is all 255 (exactly 1.0 after the gamma table)"""
    a = np.random.default_rng(k).integers(0, 256, (height, width, 3), dtype=np.uint8)
    if zero_half:
        a[:max(1, height // 2), :, :] = 0
        a[-1, -1, :] = 255
    return a


def perlin_table_a():
    """the Perlin table of the host library's two_perlin_spheres scene"""
    if not _perlin_a:
        _perlin_a.append(rt.Perlin.from_buffer_copy(rt.HostScene(3, width=16, spp=1).desc.perlins[0]))
    return _perlin_a[0]


def perlin_table_b(seed=0):
    """a Perlin table of another kind: 256 vectors uniform in [-1, 1)^3 that are NOT normalised, three permutations of 0..255"""
    rng = np.random.default_rng(0xb0b + seed)
    p = rt.Perlin()
    for i, vec in enumerate(rng.uniform(-1.0, 1.0, (256, 3))):
        p.ranvec[i] = rt.Vec3(*vec)
    for name in ("perm_x", "perm_y", "perm_z"):
        getattr(p, name)[:] = [int(x) for x in rng.permutation(256)]
    return p


def _permuted(items, order):
    if order == 1:
        return items[::-1]
    if order == 2:
        return items[1::2] + items[0::2]
    return items


def tie_scene(camera_from, order=0):
    """Every primitive has coincident copies with different materials, so every hit is an exact tie; `order` permutes the
    scan order of the world list (the winner of a tie depends on it)."""
    s = CustomScene(camera_from, spp=4, depth=6, background=(0.7, 0.8, 1.0))
    red, green, blue, white = s.lambertian(0.9, 0.1, 0.1), s.lambertian(0.1, 0.9, 0.1), s.lambertian(0.1, 0.1, 0.9), s.lambertian(0.8, 0.8, 0.8)
    mirror, glass, lamp = s.metal(0.8, 0.8, 0.3, 0.0), s.dielectric(1.5), s.light(4, 4, 4)
    back = [s.quad((-3, -3, -2), (6, 0, 0), (0, 6, 0), m) for m in (red, green, blue)]       # three coincident walls
    half = s.quad((0, -3, -2), (3, 0, 0), (0, 6, 0), mirror)                                  # coplanar, covers half of them
    floor = [s.quad((-3, -3, -2), (6, 0, 0), (0, 0, 4), m) for m in (white, red)]
    balls = [s.sphere((-1.2, -0.5, 0.0), 1.0, m) for m in (green, glass, mirror)]             # three coincident spheres
    ball2 = [s.sphere((1.3, -1.0, 0.5), 0.8, m) for m in (glass, blue)]
    top = [s.quad((-1, 2.9, -1), (2, 0, 0), (0, 0, 2), m) for m in (lamp, white)]             # a light and its opaque copy
    cube = s.translate(s.rotate_y(s.list([s.quad((-0.5, -0.5, 0.5), (1, 0, 0), (0, 1, 0), m) for m in (blue, mirror)] +
                                         [s.quad((-0.5, -0.5, -0.5), (0, 0, 1), (0, 1, 0), m) for m in (red, green)] +
                                         [s.sphere((0, 0, 0), 0.6, m) for m in (white, lamp)]), 30.0), (0.4, 1.2, 0.8))
    items = back + [half] + floor + balls + ball2 + top + [cube]
    if order == 1:
        items = items[::-1]
    elif order == 2:
        items = items[1::2] + items[0::2]
    return s.finish(s.list(items))


def single_sphere_scene(camera_from):
    s = CustomScene(camera_from, spp=4, depth=6, background=(0.7, 0.8, 1.0))
    return s.finish(s.sphere((0, 0, 0), 2.0, s.lambertian(0.5, 0.6, 0.7)))


def empty_frame_scene(camera_from):
    """A Translate around an empty list next to real geometry: the frame can never be hit."""
    s = CustomScene(camera_from, spp=4, depth=6, background=(0.7, 0.8, 1.0))
    nothing = s.translate(s.list([]), (1, 0, 0))
    return s.finish(s.list([nothing, s.sphere((0, 0, 0), 1.5, s.metal(0.7, 0.7, 0.7, 0.1)),
                            s.quad((-3, -2, -3), (6, 0, 0), (0, 0, 6), s.lambertian(0.3, 0.7, 0.3))]))


def many_spheres_scene(camera_from, n, seed=5, textured=False):
    """n small spheres (Lambertian / Metal / Dielectric) scattered over a ground sphere, as one flat HittableList: sized
    by the caller so that the compiled scene does or does not fit the LDS.  textured: the same spheres, a third of the
    materials replaced by checker, noise and image Lambertians and every fifth small sphere moving in one of MOTIONS."""
    import random
    rnd = random.Random(seed)
    s = CustomScene(camera_from, spp=4, depth=6, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(12)]
    mats += [s.metal(0.5 + 0.5 * rnd.random(), 0.5 + 0.5 * rnd.random(), 0.5 + 0.5 * rnd.random(), 0.3 * rnd.random()) for _ in range(4)]
    mats += [s.dielectric(1.5)]
    rnd2 = random.Random(seed ^ 0x7e47)  # every choice the plain scene does not make
    if textured:
        img = s.image(s.add_image(random_image(0, 13, 5)))
        na, nb = s.noise(4.0, s.add_perlin(perlin_table_a())), s.noise(1.5, s.add_perlin(perlin_table_b()))
        swap = [s.lambertian_tex(img), s.lambertian_tex(na), s.lambertian_tex(s.checker(0.3, img, nb)),
                s.lambertian_tex(s.checker(0.5, s.solid(0.9, 0.9, 0.2), s.solid(0.1, 0.2, 0.7))), s.lambertian_tex(nb)]
        for k in range(1, len(mats), 3):  # (mats[0], the ground, stays solid)
            mats[k] = swap[(k // 3) % len(swap)]
    items = [s.sphere((0.0, -1003.0, 0.0), 1000.0, mats[0])]
    for k in range(n):
        x, z = rnd.uniform(-6, 6), rnd.uniform(-6, 6)
        r = rnd.uniform(0.05, 0.25)
        y = -3.0 + r + rnd.choice([0.0, 0.0, rnd.uniform(0, 3)])
        target = None
        if textured and k % 5 == 0:
            m, size = rnd2.choice(MOTIONS), rnd2.choice([0.8, 3.0, 1e-3]) * r
            target = (x + size * m[0], y + size * m[1], z + size * m[2])
        items.append(s.sphere((x, y, z), r, rnd.choice(mats), moving_to=target))
    return s.finish(s.list(items))


def media_scene(camera_from, order=0, nested=False):
    """Participating media in every position of the scan: bounded by a sphere, by a rotated and shifted cube, by a bare
    list of quads; first, last, next to each other; overlapping each other and solid objects.  nested: one of them sits
    inside a Translate (a case the ordered layout leaves to the reference-order walk)."""
    s = CustomScene(camera_from, spp=4, depth=8, background=(0.7, 0.8, 1.0))
    red, green, white = s.lambertian(0.9, 0.2, 0.2), s.lambertian(0.2, 0.9, 0.2), s.lambertian(0.8, 0.8, 0.8)
    mirror, glass, lamp = s.metal(0.8, 0.8, 0.6, 0.05), s.dielectric(1.5), s.light(5, 5, 5)

    def cube(lo, hi, m):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
        return s.list([s.quad((x0, y0, z1), (dx, 0, 0), (0, dy, 0), m), s.quad((x1, y0, z1), (0, 0, -dz), (0, dy, 0), m),
                       s.quad((x1, y0, z0), (-dx, 0, 0), (0, dy, 0), m), s.quad((x0, y0, z0), (0, 0, dz), (0, dy, 0), m),
                       s.quad((x0, y1, z1), (dx, 0, 0), (0, 0, -dz), m), s.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), m)])

    floor = s.quad((-4, -2, -4), (8, 0, 0), (0, 0, 8), white)
    wall = s.quad((-4, -2, -3), (8, 0, 0), (0, 6, 0), red)
    light = s.quad((-1, 3.5, -1), (2, 0, 0), (0, 0, 2), lamp)
    ball, ball2 = s.sphere((-1.5, -1.0, 0.5), 1.0, glass), s.sphere((1.8, -1.2, 1.0), 0.8, mirror)
    fog_ball = s.medium(s.sphere((-1.5, -1.0, 0.5), 0.95, glass), 2.0, 0.2, 0.4, 0.9)        # inside the glass ball
    smoke = s.medium(s.translate(s.rotate_y(cube((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7), white), 25.0), (0.5, -1.0, -1.0)), 1.5, 0.05, 0.05, 0.05)
    haze = s.medium(cube((-3.5, -2.0, -2.5), (3.5, 0.0, 3.0), white), 0.15, 1.0, 1.0, 1.0)   # a bare list as the boundary
    mist = s.medium(s.sphere((0, 0, 0), 30.0, white), 0.01, 0.9, 0.9, 0.9)                    # everything is inside it
    if nested:
        smoke = s.translate(s.list([smoke]), (0.0, 0.5, 0.0))
    items = [mist, floor, ball, fog_ball, wall, smoke, haze, light, ball2, s.sphere((1.8, -1.2, 1.0), 0.8, green)]
    if order == 1:
        items = items[::-1]
    elif order == 2:
        items = items[1::2] + items[0::2]
    return s.finish(s.list(items))


def nested_frames_scene(camera_from):
    """Frames inside frames (RotateY inside Translate inside RotateY inside Translate ...), a sphere and a cube at every
    level, plus a medium whose boundary is such a nest: hits are rebuilt through up to three enclosing frames."""
    s = CustomScene(camera_from, spp=4, depth=8, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(0.8, 0.3, 0.3), s.lambertian(0.3, 0.8, 0.3), s.metal(0.7, 0.7, 0.9, 0.1), s.dielectric(1.5), s.light(3, 3, 3)]

    def cube(lo, hi, m):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
        return [s.quad((x0, y0, z1), (dx, 0, 0), (0, dy, 0), m), s.quad((x1, y0, z1), (0, 0, -dz), (0, dy, 0), m),
                s.quad((x1, y0, z0), (-dx, 0, 0), (0, dy, 0), m), s.quad((x0, y0, z0), (0, 0, dz), (0, dy, 0), m),
                s.quad((x0, y1, z1), (dx, 0, 0), (0, 0, -dz), m), s.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), m)]

    inner = s.list(cube((-0.3, -0.3, -0.3), (0.3, 0.3, 0.3), mats[2]) + [s.sphere((0.0, 0.6, 0.0), 0.25, mats[3])])
    level2 = s.list([s.translate(s.rotate_y(inner, 40.0), (0.8, 0.2, 0.0)), s.sphere((-0.5, 0.0, 0.3), 0.35, mats[0])] +
                    cube((-0.2, -0.9, -0.2), (0.2, -0.5, 0.2), mats[1]))
    level1 = s.list([s.rotate_y(s.translate(level2, (0.0, 0.5, -0.5)), -25.0), s.sphere((1.5, -0.5, 0.5), 0.4, mats[4])])
    outer = s.translate(s.rotate_y(level1, 15.0), (-0.5, 0.0, 0.0))
    smoke_nest = s.translate(s.rotate_y(s.list([s.translate(s.list(cube((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), mats[0])), (0.2, 0.0, 0.0))]), 35.0),
                             (-2.0, -1.0, 0.5))
    floor = s.quad((-4, -2, -4), (8, 0, 0), (0, 0, 8), mats[1])
    return s.finish(s.list([floor, outer, s.medium(smoke_nest, 1.2, 0.1, 0.1, 0.1), s.sphere((2.2, -1.3, -0.5), 0.7, mats[2])]))


def random_scene(camera_from, seed, textures=False):
    """A random object graph for fuzzing the two walks against the oracle: spheres, quads and cubes, alone or grouped
    in (nested) Translate / RotateY frames, media bounded by spheres, cubes and framed cubes at random places of the
    world list, some objects duplicated exactly (ties), random materials.  textures: the same graph (the first generator's
    stream is untouched), with materials also drawn from textured Lambertians, lights and isotropic albedos and spheres
    that move with probability 0.3 — every such choice comes from a second generator."""
    import random
    rnd = random.Random(seed)
    rnd2 = random.Random(seed ^ 0x7e47)
    s = CustomScene(camera_from, spp=2, depth=6, background=(0.7, 0.8, 1.0) if rnd.random() < 0.7 else (0.0, 0.0, 0.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(4)]
    mats += [s.metal(rnd.random(), rnd.random(), rnd.random(), rnd.choice([0.0, 0.3, 1.5])), s.dielectric(rnd.choice([1.5, 1.0 / 1.5, 2.4])),
             s.light(rnd.uniform(1, 8), rnd.uniform(1, 8), rnd.uniform(1, 8))]
    tex_mats, tex_pool = [], []
    if textures:
        imgs = [s.image(s.add_image(random_image(seed * 4 + k, w, h))) for k, (w, h) in enumerate(rnd2.sample(IMAGE_SIZES, 2))]
        noises = [s.noise(rnd2.choice([0.5, 4.0]), s.add_perlin(perlin_table_a())), s.noise(rnd2.choice([1.5, 9.0]), s.add_perlin(perlin_table_b(seed)))]
        flat = s.solid(rnd2.random(), rnd2.random(), rnd2.random())
        chk = s.checker(rnd2.uniform(0.1, 0.9), rnd2.choice(imgs), rnd2.choice(noises))
        deep = s.checker(rnd2.uniform(0.3, 1.5), s.checker(rnd2.uniform(0.1, 0.5), flat, chk), rnd2.choice(imgs + noises))
        tex_pool = imgs + noises + [chk, deep]
        tex_mats = [s.lambertian_tex(t) for t in tex_pool] + [s.light_tex(rnd2.choice(tex_pool)), s.light_tex(deep)]

    def pick(m):
        """m (the first generator's choice), or a textured material in its place"""
        return rnd2.choice(tex_mats) if textures and rnd2.random() < 0.45 else m

    def target(center, radius):
        """where a sphere moves to (None: it stays)"""
        if not textures or rnd2.random() >= 0.3:
            return None
        m, size = rnd2.choice(MOTIONS), rnd2.choice([0.5, 3.0, 1e-3]) * radius
        return (center[0] + size * m[0], center[1] + size * m[1], center[2] + size * m[2])

    def pos(scale=2.5):
        return (rnd.uniform(-scale, scale), rnd.uniform(-scale, scale), rnd.uniform(-scale, scale))

    def cube(m):
        x0, y0, z0 = pos(2.0)
        dx, dy, dz = rnd.uniform(0.2, 1.2), rnd.uniform(0.2, 1.2), rnd.uniform(0.2, 1.2)
        x1, y1, z1 = x0 + dx, y0 + dy, z0 + dz
        return [s.quad((x0, y0, z1), (dx, 0, 0), (0, dy, 0), m), s.quad((x1, y0, z1), (0, 0, -dz), (0, dy, 0), m),
                s.quad((x1, y0, z0), (-dx, 0, 0), (0, dy, 0), m), s.quad((x0, y0, z0), (0, 0, dz), (0, dy, 0), m),
                s.quad((x0, y1, z1), (dx, 0, 0), (0, 0, -dz), m), s.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), m)]

    def solid(depth):
        kind = rnd.choice(["sphere", "sphere", "quad", "cube", "group"] if depth < 2 else ["sphere", "quad", "cube"])
        m = pick(rnd.choice(mats))
        if kind == "sphere":
            c, r = pos(), rnd.uniform(0.15, 0.9)
            return [s.sphere(c, r, m, moving_to=target(c, r))]
        if kind == "quad":
            q = pos()
            u, v = (rnd.uniform(-1.5, 1.5), rnd.uniform(-0.3, 0.3), rnd.uniform(-1.5, 1.5)), (rnd.uniform(-0.3, 0.3), rnd.uniform(0.3, 1.5), rnd.uniform(-0.3, 0.3))
            return [s.quad(q, u, v, m)]
        if kind == "cube":
            return [s.list(cube(m))] if rnd.random() < 0.5 else cube(m)
        items = [r for _ in range(rnd.randint(0, 3)) for r in solid(depth + 1)]
        g = s.list(items)
        wrap = rnd.choice(["t", "r", "tr", "rt"])
        for w in wrap:
            g = s.translate(g, pos(1.0)) if w == "t" else s.rotate_y(g, rnd.uniform(-80, 80))
        return [g]

    items = []
    for _ in range(rnd.randint(1, 9)):
        roll = rnd.random()
        if roll < 0.2:
            boundary = rnd.choice(["sphere", "cube", "framed"])
            if boundary == "sphere":
                c, r = pos(), rnd.uniform(0.5, 3.0)
                b = s.sphere(c, r, mats[0], moving_to=target(c, r))
            elif boundary == "cube":
                b = s.list(cube(mats[0]))
            else:
                b = s.translate(s.rotate_y(s.list(cube(mats[0])), rnd.uniform(-60, 60)), pos(1.0))
            density, colour = rnd.choice([0.05, 0.5, 3.0]), (rnd.random(), rnd.random(), rnd.random())
            items.append(s.medium(b, density, *colour, texture=rnd2.choice(tex_pool) if textures and rnd2.random() < 0.5 else None))
        else:
            new = solid(0)
            items.extend(new)
            if rnd.random() < 0.15 and new:  # an exact copy right after, or at the end: ties
                dup = new[0]
                if dup.kind == rt.RT_HITTABLE_SPHERE:
                    sp = s.spheres[dup.index]
                    items.insert(rnd.randint(0, len(items)), s.sphere((sp.center.x, sp.center.y, sp.center.z), sp.radius, pick(rnd.choice(mats))))
                    if sp.is_moving:  # the copy moves with the original: the tie holds at every time
                        s.spheres[-1].center_vec, s.spheres[-1].is_moving = sp.center_vec, 1
                elif dup.kind == rt.RT_HITTABLE_QUAD:
                    qd = s.quads[dup.index]
                    items.insert(rnd.randint(0, len(items)), s.quad(qd.q.tuple(), qd.u.tuple(), qd.v.tuple(), pick(rnd.choice(mats))))
    return s.finish(s.list(items))


def many_media_scene(camera_from, n=40, seed=11):
    """n solid spheres alternating with n sphere-bounded media in one flat list: 2n + steps of the world sequence, more than
    the ordered layout's kernel keeps (ORDERED_MAX_STEPS = 64), so the scene compiler turns the ordered layout down and the
    reference-order walk must find every medium's boundary sphere where the threaded layout put it."""
    import random
    rnd = random.Random(seed)
    s = CustomScene(camera_from, spp=4, depth=6, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(5)] + [s.metal(0.8, 0.8, 0.8, 0.1), s.dielectric(1.5)]
    items = []
    for _ in range(n):
        items.append(s.sphere((rnd.uniform(-4, 4), rnd.uniform(-2, 2), rnd.uniform(-4, 4)), rnd.uniform(0.2, 0.6), rnd.choice(mats)))
        boundary = s.sphere((rnd.uniform(-4, 4), rnd.uniform(-2, 2), rnd.uniform(-4, 4)), rnd.uniform(0.3, 1.2), mats[0])
        items.append(s.medium(boundary, rnd.choice([0.3, 1.0, 4.0]), rnd.random(), rnd.random(), rnd.random()))
    return s.finish(s.list(items))


def many_instances_scene(camera_from, n, seed=3, spheres=True):
    """n rotated and shifted cubes (each a Translate(RotateY(list of six quads))) beside each other over a floor, some
    overlapping, two of them nested once more — the walk meets many instances per ray.  n <= 32: the world frame's
    instances are walked after its own tree (one bit each); n > 32: entered where the walk meets them.
    spheres=False: quads only, so that the quads + frames kernel renders it (the one that defers instances)."""
    import random
    rnd = random.Random(seed)
    s = CustomScene(camera_from, spp=4, depth=6, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(0.8, 0.3, 0.3), s.lambertian(0.3, 0.8, 0.3), s.metal(0.7, 0.7, 0.9, 0.2), s.light(2, 2, 2)]

    def cube(h, m):
        return [s.quad((-h, -h, h), (2 * h, 0, 0), (0, 2 * h, 0), m), s.quad((h, -h, h), (0, 0, -2 * h), (0, 2 * h, 0), m),
                s.quad((h, -h, -h), (-2 * h, 0, 0), (0, 2 * h, 0), m), s.quad((-h, -h, -h), (0, 0, 2 * h), (0, 2 * h, 0), m),
                s.quad((-h, h, h), (2 * h, 0, 0), (0, 0, -2 * h), m), s.quad((-h, -h, -h), (2 * h, 0, 0), (0, 0, 2 * h), m)]

    side = max(1, int(math.ceil(math.sqrt(n))))
    world = [s.quad((-6, -1.5, -6), (12, 0, 0), (0, 0, 12), mats[1]),
             s.sphere((0.0, 2.5, 0.0), 0.6, mats[3]) if spheres else s.quad((-0.6, 2.5, -0.6), (1.2, 0, 0), (0, 0, 1.2), mats[3])]
    for k in range(n):
        gx, gz = k % side, k // side
        h = rnd.uniform(0.15, 0.45)
        inner = s.list(cube(h, mats[k % 3]))
        if k % 7 == 3:  # one more frame inside
            extra = s.sphere((0.0, -0.4, 0.0), 0.2, mats[2]) if spheres else s.quad((-0.2, -0.4, -0.2), (0.4, 0, 0), (0, 0, 0.4), mats[2])
            inner = s.list([s.translate(s.rotate_y(inner, rnd.uniform(-60, 60)), (0.1, 0.2, 0.0)), extra])
        pos = ((gx - side / 2) * 0.9 + rnd.uniform(-0.3, 0.3), rnd.uniform(-1.0, 0.5), (gz - side / 2) * 0.9 + rnd.uniform(-0.3, 0.3))
        world.append(s.translate(s.rotate_y(inner, rnd.uniform(-90, 90)), pos))
    return s.finish(s.list(world))


def many_materials_scene(camera_from, n_lambertian, depth=12):
    """n_lambertian + 2 materials, few of them used but those spread over the whole range: with 65 535 or more, a parked attenuation's
    16-bit material index no longer names them all and the scene is rendered by the kernels that park colours (rt_api.cpp ids_ok = 0).
    (The scene of tests/test_gpu_ties.py test_more_materials_than_a_parked_index_can_name.)"""
    import random
    rnd = random.Random(3)
    s = CustomScene(camera_from, spp=4, depth=depth, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(n_lambertian)]
    mats += [s.metal(0.9, 0.8, 0.7, 0.1), s.dielectric(1.5)]
    n = len(mats)
    pick = [mats[0], mats[1], mats[65530], mats[65531], mats[n // 2], mats[n - 4], mats[n - 3], mats[n - 2], mats[n - 1]]
    items = [s.sphere((0.0, -1003.0, 0.0), 1000.0, mats[40000])]
    for k in range(40):
        items.append(s.sphere((rnd.uniform(-4, 4), rnd.uniform(-2.5, 1.5), rnd.uniform(-4, 2)), rnd.uniform(0.3, 0.8), pick[k % len(pick)]))
    items.append(s.quad((-5.0, -3.0, -5.0), (10.0, 0.0, 0.0), (0.0, 6.0, 0.0), mats[n - 5]))
    return s.finish(s.list(items))


def _cube(s, lo, hi, mats):
    """the six quads of Quad::cube; mats: one material, or six"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
    m = mats if isinstance(mats, (list, tuple)) else [mats] * 6
    return [s.quad((x0, y0, z1), (dx, 0, 0), (0, dy, 0), m[0]), s.quad((x1, y0, z1), (0, 0, -dz), (0, dy, 0), m[1]),
            s.quad((x1, y0, z0), (-dx, 0, 0), (0, dy, 0), m[2]), s.quad((x0, y0, z0), (0, 0, dz), (0, dy, 0), m[3]),
            s.quad((x0, y1, z1), (dx, 0, 0), (0, 0, -dz), m[4]), s.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), m[5])]


def textured_scene(camera_from, frames, order=0):
    """Checker, noise and image textures where the stock scenes have none: images on an axis-aligned quad and on a skewed
    parallelogram, on a still and on a moving sphere; noise of two Perlin tables at two scales; checkers of checkers (three levels)
    with image and noise cells; a light that emits a checker of (an image with texels of exactly zero, a solid); five images of
    IMAGE_SIZES.  The objects sit in all eight octants (checker floor and Perlin `& 255` of negative integers).
    frames=False: spheres, quads and one flat list, nothing else.  frames=True: also textured objects inside Translate(RotateY(...)),
    one such frame inside another, and two media with textured albedos.  `order` permutes the world list as tie_scene does."""
    s = CustomScene(camera_from, spp=4, depth=8, background=(0.7, 0.8, 1.0))
    img = [s.image(s.add_image(random_image(k, w, h, zero_half=(k == 2)))) for k, (w, h) in enumerate(IMAGE_SIZES)]
    pa, pb = s.add_perlin(perlin_table_a()), s.add_perlin(perlin_table_b())
    noise_a, noise_b = s.noise(4.0, pa), s.noise(1.5, pb)
    grey, blue, lamp_white = s.solid(0.7, 0.7, 0.7), s.solid(0.1, 0.2, 0.8), s.solid(4.0, 4.0, 4.0)
    m_img = [s.lambertian_tex(t) for t in img]
    m_noise_a, m_noise_b = s.lambertian_tex(noise_a), s.lambertian_tex(noise_b)
    m_floor = s.lambertian_tex(s.checker(0.8, s.checker(0.3, img[0], noise_a), grey))
    m_deep = s.lambertian_tex(s.checker(1.0, s.checker(0.5, s.checker(0.25, img[2], blue), noise_b), s.checker(0.4, grey, img[4])))
    m_lamp = s.light_tex(s.checker(0.5, img[2], lamp_white))
    items = [
        s.quad((-4.0, -2.5, -4.0), (8.0, 0.0, 0.0), (0.0, 0.0, 8.0), m_floor),                      # the floor: y < 0, x and z of both signs
        s.quad((-3.6, -1.0, -3.0), (2.4, 0.0, 0.0), (0.0, 2.0, 0.0), m_img[0]),                      # axis-aligned, 13x5
        s.quad((0.2, 0.3, -2.5), (2.2, 0.5, 0.3), (0.8, 1.8, -0.4), m_img[2]),                       # skewed: u . v != 0, so w matters
        s.quad((1.2, -2.3, -1.5), (2.0, 0.0, 0.5), (0.0, 1.6, 0.0), m_noise_b),                      # noise on a quad
        s.sphere((-1.8, -1.2, 1.0), 0.8, m_img[0]),                                                  # image on a still sphere
        s.sphere((1.6, 1.5, 0.8), 0.6, m_img[0], moving_to=(2.1, 1.2, 1.0)),                        # ... on a moving one: UV from the moved centre
        s.sphere((-2.2, 1.6, -0.5), 0.9, m_noise_a),
        s.sphere((0.3, -1.4, 2.0), 0.7, m_noise_b, moving_to=(0.3 - 0.6, -1.4 + 0.2, 2.0 + 0.5)),
        s.sphere((2.3, -0.3, -0.8), 0.9, m_deep),
        s.sphere((-1.0, 1.0, 1.5), 0.4, m_img[1]),                                                   # 1x1
        s.sphere((-2.6, 0.2, 1.2), 0.45, m_img[3]),                                                  # 1x9
        s.sphere((0.9, 0.4, 2.2), 0.4, m_img[4]),                                                    # 17x1
        s.quad((-1.2, 2.2, -1.0), (2.4, 0.0, 0.0), (0.0, 0.6, 1.6), m_lamp),                         # the light, tilted towards the camera
    ]
    if frames:
        cube_mats = [m_img[0], m_noise_a, m_img[2], m_deep, m_img[4], m_floor]
        group = s.list(_cube(s, (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), cube_mats) +
                       [s.sphere((0.0, 0.95, 0.0), 0.4, m_img[0]), s.sphere((0.9, 0.0, 0.3), 0.3, m_img[3], moving_to=(1.1, 0.4, -0.2))])
        items.append(s.translate(s.rotate_y(group, 35.0), (-0.4, -0.6, 0.2)))
        inner = s.translate(s.rotate_y(s.list([s.quad((-0.4, -0.4, 0.0), (0.8, 0.1, 0.0), (0.2, 0.8, 0.1), m_img[0]),
                                               s.sphere((0.0, 0.0, -0.5), 0.35, m_noise_b)]), -50.0), (0.3, 0.2, 0.0))
        outer = s.list([inner, s.sphere((-0.6, 0.3, 0.0), 0.3, m_deep, moving_to=(-0.6, 0.5, 0.3))])
        items.append(s.translate(s.rotate_y(outer, 20.0), (1.2, 2.0, -1.0)))
        items.append(s.medium(s.sphere((-2.8, -1.4, -1.0), 0.9, m_img[1]), 1.5, texture=s.checker(0.35, noise_a, img[0])))
        items.append(s.medium(s.list(_cube(s, (2.4, -2.4, 0.6), (3.6, -1.2, 1.8), m_img[1])), 2.0, texture=noise_b))
    return s.finish(s.list(_permuted(items, order)))


def moving_scene(camera_from, n=40, frames=True, seed=9):
    """A ground and n spheres of which most move: sphere k to its centre + size * MOTIONS[k % 14], the size cycling through 0.8, 3 and
    1e-3 radii; every ninth stays still.  Beside them: two exact coincident moving copies with different materials; a moving glass
    sphere around a still medium; a medium whose boundary is a sphere moving along (0.5, 0.5, 0) — further than its radius — as the
    medium's own record; a medium bounded by a moving sphere inside a one-item list; with `frames`, two moving spheres inside
    Translate(RotateY(...))."""
    import random
    rnd = random.Random(seed)
    s = CustomScene(camera_from, spp=4, depth=8, background=(0.7, 0.8, 1.0))
    mats = [s.lambertian(rnd.random(), rnd.random(), rnd.random()) for _ in range(5)] + [s.metal(0.8, 0.8, 0.7, 0.1), s.dielectric(1.5)]
    glass = mats[-1]
    items = [s.sphere((0.0, -1003.0, 0.0), 1000.0, mats[0])]
    for k in range(n):
        c, r = (rnd.uniform(-3.0, 3.0), rnd.uniform(-2.2, 2.0), rnd.uniform(-2.5, 2.5)), rnd.uniform(0.2, 0.5)
        m, size = MOTIONS[k % 14], (0.8, 3.0, 1e-3)[(k + k // 14) % 3] * r
        still = k % 9 == 4
        items.append(s.sphere(c, r, mats[k % len(mats)], moving_to=None if still else (c[0] + size * m[0], c[1] + size * m[1], c[2] + size * m[2])))
    items += [s.sphere((-2.0, 2.2, 0.5), 0.45, m, moving_to=(-1.4, 1.9, 0.9)) for m in (mats[1], mats[5])]     # a tie at every time
    items.append(s.sphere((2.2, 1.8, 0.0), 0.7, glass, moving_to=(2.35, 1.8, 0.0)))
    items.append(s.medium(s.sphere((2.2, 1.8, 0.0), 0.5, glass), 3.0, 0.2, 0.4, 0.9))                          # still, inside the moving glass
    items.append(s.medium(s.sphere((-0.5, -1.0, 1.5), 0.3, glass, moving_to=(0.0, -0.5, 1.5)), 4.0, 0.9, 0.3, 0.2))
    items.append(s.medium(s.list([s.sphere((0.8, 0.2, 1.8), 0.4, glass, moving_to=(0.1, 0.2, 2.4))]), 2.5, 0.1, 0.1, 0.1))
    if frames:
        pair = s.list([s.sphere((0.0, 0.0, 0.0), 0.4, mats[2], moving_to=(0.9, -0.3, 0.5)), s.sphere((0.0, 0.9, 0.0), 0.3, mats[5], moving_to=(-0.4, 0.9, -0.8))])
        items.append(s.translate(s.rotate_y(pair, 40.0), (-2.4, -0.2, 1.2)))
    return s.finish(s.list(items))


def without_motion(scene):
    """the same scene (a CustomScene) with every sphere at its time-0 place: a description that shares every table but the spheres"""
    spheres = (rt.Sphere * max(1, scene.desc.n_spheres))()
    for i in range(scene.desc.n_spheres):
        spheres[i] = rt.Sphere.from_buffer_copy(scene.desc.spheres[i])
        spheres[i].center_vec, spheres[i].is_moving = _v(0, 0, 0), 0
    still = CustomScene.__new__(CustomScene)
    still.camera, still._keep, still._spheres = scene.camera, scene._keep, spheres
    still.desc = rt.SceneDesc.from_buffer_copy(scene.desc)
    still.desc.spheres = spheres
    return still
