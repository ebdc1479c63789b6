"""The scene plan against the device: a scene created from a description reports the plan's stats, and a render of it runs the kernel
and starts its queries where the plan (rt_debug_scene_plan, computed without a device) says — for each stock scene under the three
walks, with the LDS and (use_lds = 0) without it."""
import numpy as np
import pytest

import scene_plan_cases as spc

pytestmark = pytest.mark.gpu

CASES = [(name, option_set, use_lds) for name in spc.STOCK for option_set in spc.OPTION_SETS for use_lds in (-1, 0)]


@pytest.mark.parametrize("name,option_set,use_lds", CASES, ids=lambda v: str(v))
def test_scene_and_launch_are_the_plans(rt, gpu, name, option_set, use_lds):
    hs = spc.scene(rt, name, width=16)
    opts = spc.options(rt, option_set, use_lds=use_lds)
    plan = rt.debug_scene_plan(hs, **opts)
    scene = rt.DeviceScene(hs, **opts)
    try:
        assert scene.stats() == plan["stats"]
        frame = scene.render(rt.render_params(seed=3, sample_end=1, max_depth=4))
        assert np.all(np.isfinite(frame))
        lds = plan["lds_level"] if use_lds != 0 else 0
        level = plan["levels"][lds]
        k = rt.debug_last_kernel()
        assert {n: k[n] for n in ("features", "lds_level", "ordered", "wide", "aux", "threads")} == \
            dict(features=level["features"], lds_level=lds, ordered=plan["ordered"], wide=plan["wide"], aux=level["aux_in_lds"], threads=level["threads"])
        # as launch_render reports them: the stage and the inline word only on the library's own trees, under the default start_shortcut
        # and start_inline (1); the inline test is asked for where the start leaf is one sphere
        one_sphere = plan["o_start_stage"] == 1 and plan["o_start_end"] == plan["o_start_prim"] + 1
        assert rt.debug_last_start() | {"ran_inline": None} == dict(
            stage=plan["o_start_stage"] if plan["ordered"] else 0, first=plan["o_start_prim"], end=plan["o_start_end"],
            start_inline=int(bool(plan["ordered"] and one_sphere)), ran_inline=None)
    finally:
        scene.close()
