"""The host side of rt_render_views (no GPU): rth_scene_camera_look — Camera::new over the scene's own CameraSettings with other look
points —, the ctypes mirror of rt_view, and the new symbols of both shared libraries."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("scene", range(9))
def test_camera_look_without_points_is_the_scenes_camera(rt, scene):
    hs = rt.HostScene(scene, width=64, spp=4, depth=8, earth_image="synthetic:64x32")
    assert bytes(rt.camera_look(hs)) == bytes(hs.camera)
    look_from, look_at, _ = rt.scene_look(hs)
    assert bytes(rt.camera_look(hs, look_from, look_at)) == bytes(hs.camera)
    assert bytes(rt.camera_look(hs, look_from=[look_from[0] + 1.0, look_from[1], look_from[2]])) != bytes(hs.camera)


def vec(v):
    return np.array([v.x, v.y, v.z])


@pytest.mark.parametrize("scene", [0, 6, 8])
def test_a_half_turn_mirrors_the_camera_through_the_axis(rt, scene):
    hs = rt.HostScene(scene, width=64, spp=4, depth=8, earth_image="synthetic:64x32")
    look_from, look_at, vup = (np.array(v) for v in rt.scene_look(hs))
    turned = np.array(rt.orbit_look_from(hs, 1, 2))
    cam = rt.camera_look(hs, turned)
    # center = look_from: its mirror image through the axis (look_at + t vup) is 2 (foot of the perpendicular) - center
    axis = vup / np.sqrt(vup @ vup)
    p = look_from - look_at
    mirrored = look_at + 2.0 * (axis @ p) * axis - p
    scale = np.abs(look_from).max() + np.abs(look_at).max()
    assert np.abs(vec(cam.center) - mirrored).max() <= 8 * np.finfo(float).eps * scale, (vec(cam.center), mirrored)
    # u = vup x w turns with w: pixel_delta_u is negated, to within a few ulp of its largest component
    du, du0 = vec(cam.pixel_delta_u), vec(hs.camera.pixel_delta_u)
    assert np.abs(du + du0).max() <= 8 * np.finfo(float).eps * np.abs(du0).max(), (du, du0)
    assert (cam.image_width, cam.image_height, cam.samples_per_pixel, cam.max_depth) == \
        (hs.camera.image_width, hs.camera.image_height, hs.camera.samples_per_pixel, hs.camera.max_depth)
    assert cam.background.tuple() == hs.camera.background.tuple() and cam.defocus_angle == hs.camera.defocus_angle
    # a whole turn in steps: view 0 of any orbit is the scene's own camera
    assert bytes(rt.orbit_views(hs, 4, 7)[0].camera) == bytes(hs.camera)
    assert [v.seed for v in rt.orbit_views(hs, 4, 7)] == [7, 8, 9, 10]


def rotated(look_from, look_at, vup, degrees):
    """look_from turned about the axis through look_at along vup, counter-clockwise seen from vup's tip: the rotation matrix
    I + sin K + (1 - cos) K^2 of the axis' cross-product matrix K, not the library's own formula"""
    a = vup / np.sqrt(vup @ vup)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.deg2rad(degrees)
    return look_at + (np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)) @ (look_from - look_at)


@pytest.mark.parametrize("scene", [0, 6, 8])
@pytest.mark.parametrize("k, n", [(1, 3), (2, 3), (1, 4), (7, 30)])
def test_orbit_look_from_turns_the_right_way_about_the_right_axis(rt, scene, k, n):
    """a turn the wrong way, or about another axis, is off by about the orbit's radius; rounding is a few ulp of the coordinates"""
    hs = rt.HostScene(scene, width=64, spp=4, depth=8, earth_image="synthetic:64x32")
    look_from, look_at, vup = (np.array(v) for v in rt.scene_look(hs))
    got = np.array(rt.orbit_look_from(hs, k, n))
    want = rotated(look_from, look_at, vup, 360.0 * k / n)
    scale = np.abs(look_from).max() + np.abs(look_at).max()
    assert np.abs(got - want).max() <= 16 * np.finfo(float).eps * scale, (got, want)
    assert np.abs(got - look_from).max() > 1e-3 * scale
    assert rt.orbit_look_from(hs, 0, n) == tuple(look_from)


def test_rt_view_matches_the_c_layout(rt, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_host.h"', "int main(void){",
             'printf("rt_view %zu\\n", sizeof(rt_view));']
    for fname, _ in rt.View._fields_:
        lines.append(f'printf("rt_view.{fname} %zu\\n", offsetof(rt_view, {fname}));')
    lines.append('printf("max_tiles %lld\\n", (long long)RT_VIEWS_MAX_TILES);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["rt_view"]) == C.sizeof(rt.View)
    for fname, _ in rt.View._fields_:
        assert int(got[f"rt_view.{fname}"]) == getattr(rt.View, fname).offset, fname
    assert int(got["max_tiles"]) == min(1 << 27, (1 << 31) // 64)


def test_both_libraries_export_the_new_symbols(rt):
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines()}
    assert {"rt_render_views", "rt_render_views_device"} <= exported(rt.LIB_DIR / "librt_amd.so")
    assert {"rth_scene_camera_look", "rth_scene_look", "rth_scene_orbit_look_from"} <= exported(rt.LIB_DIR / "librt_host.so")
    assert "rt_render_views" in rt.RT_AMD_SYMBOLS and "rth_scene_camera_look" in rt.RT_HOST_SYMBOLS
