"""k_surface_scatter and the next-event kernel reading the material and instance tables from a copy in LDS (RAYHIP_SHADE_LDS_TABLES=1, the
default) against the same kernels reading them from memory (RAYHIP_SHADE_LDS_TABLES=0): the same fields and the same values from another
place, so the frames must agree bit for bit.  Needs a real MI355X."""
import struct

import numpy as np
import pytest

import util
from ray_amd import hip

pytestmark = pytest.mark.gpu

SCENES = ["cornell_basic", "cornell_principled", "cornell_lights", "cornell_env", "cornell_instances"]
SWITCHES = ("RAYHIP_SHADE_LDS_TABLES", "RAYHIP_SHADE_LDS_MATERIALS_MAX", "RAYHIP_SHADE_LDS_INSTANCES_MAX", "RAYHIP_SURFACE_PARK")


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


def table_counts(name):
    """(materials, mesh instances) of a golden scene, from the section table of its blob (ray_amd/csrc/scene_blob.h)"""
    blob = util.golden_scene(name)
    assert blob[:8] == b"RAYHIPS1"
    (n_sections,) = struct.unpack_from("<I", blob, 8)
    size = {}
    for k in range(n_sections):
        sec_name, _, sec_size = struct.unpack_from("<24sQQ", blob, 16 + 40 * k)
        size[sec_name.rstrip(b"\0").decode()] = sec_size
    assert size["materials"] % 76 == 0 and size["mesh_instances"] % 144 == 0
    return size["materials"] // 76, size["mesh_instances"] // 144


_frames = {}


def frames(lib, monkeypatch, name, **env):
    """round 6's form pinned (RAYHIP_SHADE_SPLIT=29: the Cornell boxes would otherwise take the three-kernel form and never run the fused kernel);
    five iterations batched and two single ones, so bounce 0 and the later bounces both run.  One render per (scene, switches)."""
    key = (name, tuple(sorted(env.items())))
    if key not in _frames:
        monkeypatch.setenv("RAYHIP_SHADE_SPLIT", "29")
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        ctx = util.make_context(lib, name)
        ctx.render_batch(1, 5)
        ctx.render(6)
        ctx.render(7)
        _frames[key] = (ctx.readback(hip.BUF_RAW), ctx.readback(hip.BUF_BASE_COLOR), ctx.readback(hip.BUF_DEPTH_NORMALS))
    return _frames[key]


def assert_same(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("name", SCENES)
def test_lds_tables_on_and_off_agree(gpu_lib, name, monkeypatch):
    """cornell_principled walks mix chains through the table, cornell_instances holds several instances with non-identity transforms"""
    off = frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_TABLES=0)
    assert_same(frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_TABLES=1), off, name)
    assert_same(frames(gpu_lib, monkeypatch, name), off, name + " (default)")


@pytest.mark.parametrize("name", SCENES)
def test_material_cap_boundary(gpu_lib, name, monkeypatch):
    """a cap equal to the scene's material count still takes the LDS form, one below it falls back to the tables in memory"""
    n_materials, _ = table_counts(name)
    assert n_materials >= 1
    off = frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_TABLES=0)
    for cap in (n_materials, n_materials - 1):
        assert_same(frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_MATERIALS_MAX=cap), off, (name, cap))


def test_instance_cap_boundary(gpu_lib, monkeypatch):
    name = "cornell_instances"
    _, n_instances = table_counts(name)
    assert n_instances > 1, "the scene is there for its several instances"
    off = frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_TABLES=0)
    for cap in (n_instances, n_instances - 1):
        assert_same(frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_INSTANCES_MAX=cap), off, (name, cap))


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("park", [0, 1])
def test_parked_and_unparked_with_lds_tables(gpu_lib, name, park, monkeypatch):
    """the table region and the park slots are separate LDS arrays: the parked kernel with the tables must not see one through the other"""
    off = frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_TABLES=0)
    assert_same(frames(gpu_lib, monkeypatch, name, RAYHIP_SHADE_LDS_TABLES=1, RAYHIP_SURFACE_PARK=park), off, (name, park))
