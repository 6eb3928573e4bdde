"""k_surface_scatter with the ray and the pick parked in LDS (RAYHIP_SURFACE_PARK=1, the default) against the same kernel holding them in
registers (RAYHIP_SURFACE_PARK=0): the same per-lane arithmetic, so the frames must agree bit for bit.  Needs a real MI355X."""
import numpy as np
import pytest

import util
from ray_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


@pytest.mark.parametrize("name", ["cornell_lights", "cornell_principled", "cornell_env", "cornell_basic", "cornell_instances"])
def test_parked_and_unparked_surface_scatter_agree(gpu_lib, name, monkeypatch):
    """round 6's form pinned (RAYHIP_SHADE_SPLIT=29: the Cornell boxes would otherwise take the three-kernel form and never run the fused
    kernel); five iterations batched and two single ones, so bounce 0 and the later bounces both run"""
    monkeypatch.setenv("RAYHIP_SHADE_SPLIT", "29")
    frames = {}
    for park in ("1", "0"):
        monkeypatch.setenv("RAYHIP_SURFACE_PARK", park)
        ctx = util.make_context(gpu_lib, name)
        ctx.render_batch(1, 5)
        ctx.render(6)
        ctx.render(7)
        frames[park] = (ctx.readback(hip.BUF_RAW), ctx.readback(hip.BUF_BASE_COLOR), ctx.readback(hip.BUF_DEPTH_NORMALS))
    for a, b in zip(frames["1"], frames["0"]):
        assert np.array_equal(a, b), name
