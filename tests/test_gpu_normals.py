"""Normal sets on the device (rayhip_normals_create / _destroy): while a set is live, every call that writes the vertex array recomputes
the normals and / or bitangents of the set's range in place, behind its copy and ahead of the refit (ray_amd/csrc/normals.h,
normals.hip.h).

What is asserted: after every such call the device's vertex array equals the host build of the same element functions
(tests/hostsim/hostsim_normals.cpp) bit for bit; a bitangent set at the upload pose leaves the bitangents the reference's scene build
derived bytewise as they are; arrays and frames equal those of a context that got the host-built records through update_vertices with
no set -- the same arrays under the same trees, so no tolerance; every refusal leaves the vertex array as it was; and with no live set
the trace of an update is what it was.  The scene is normals_cases.cloth (3760 vertices in use: the sheet alone is eleven blocks)."""
import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import morph_cases as M
import normals_cases as NC
import skin_cases as S
import util
import vertex_update_cases as V
from ray_amd import hip

pytestmark = [pytest.mark.gpu]

W, H, SPP = 96, 64, 4
bits = NC.bits
N, B = NC.N, NC.B


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    assert NC.have_normals_lib() and M.have_morph_lib() and S.have_skin_lib() and V.have_refit_lib(), "tests/hostsim is not built (run __graft_entry__.build())"
    return lib


@pytest.fixture(scope="module")
def cloth():
    """(blob, arrays, meshes, reachable triangles) of the scene: built once, never changed"""
    blob, a, meshes = NC.scene()
    return blob, a, meshes, NC.reachable(a)


def _context(lib, blob=None, refit=False):
    ctx = hip.Context(0, lib)
    ctx.upload_static(util.pmj())
    ctx.resize(W, H)
    if refit:
        ctx.refit_lights(True)
    if blob is not None:
        ctx.upload_scene_blob(blob)
    return ctx


def _frames(ctx):
    ctx.clear()
    return util.render_frames(ctx, SPP).copy()


def _accel(ctx, kinds=(0, 1, 2, 4)):
    return [ctx.read_accel(k).copy() for k in kinds]


def _same(x, y):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))


def _on_device(array):
    t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


class Set:
    """a normal set of the tests: range, flags, weld (by position at the upload pose) or none"""

    def __init__(self, a, first, count, flags, weld=False):
        self.first, self.count, self.flags = int(first), int(count), flags
        self.weld = hip.weld_by_position(a.vertices["p"][first:first + count]) if weld else None

    def create(self, ctx):
        return ctx.create_normals(self.first, self.count, bool(self.flags & N), bool(self.flags & B), self.weld)


def _recomputed(a, tris, vertices, sets):
    """the vertex array after the live `sets` were recomputed over `vertices` (the host build; the sets do not depend on each other)"""
    v = vertices
    for s in sets:
        v = NC.host_recompute(a, v, tris, s.first, s.count, s.flags, s.weld)
    return v


def _sets(a, meshes):
    """ranges 1, 255, 256 and 257 vertices long inside the sheet (none begins at a multiple of 64), the fan, whose hub's row is longer than
    a chunk of the kernel, and the welded sphere: six sets at once"""
    sheet, fan, sphere = meshes["sheet"], meshes["fan"], meshes["sphere"]
    return [Set(a, sheet.first + 3, 1, N | B), Set(a, sheet.first + 10, 255, N), Set(a, sheet.first + 300, 256, B), Set(a, sheet.first + 601, 257, N | B, weld=True),
            Set(a, fan.first, fan.count, N | B), Set(a, sphere.first, sphere.count, N | B, weld=True)]


def _skin_and_morph(a, meshes):
    """a skin from the sheet's first vertex to the fan's last (it holds four of the sets and the fan's) and a morph set WITHOUT normal or
    bitangent deltas over the sphere"""
    sheet, fan, sphere = meshes["sheet"], meshes["fan"], meshes["sphere"]
    skin = S.Skin(a, sheet.first, fan.first + fan.count - sheet.first, 3, 4)
    rng = np.random.RandomState(9)
    every = np.arange(sphere.count, dtype=np.uint32)
    ms = M.MorphSet(a, sphere.first, sphere.count, [M._target(rng, every, S.extent(a), 0.3, with_frame=False), M._target(rng, every[::3], S.extent(a), 0.3, with_frame=False)])
    return skin, ms


@pytest.mark.parametrize("path", ("update_vertices", "update_vertices_device", "pose_skins", "pose"))
def test_every_writing_call_recomputes_the_live_sets(gpu_lib, cloth, path):
    blob, a, meshes, tris = cloth
    sets = _sets(a, meshes)
    skin, ms = _skin_and_morph(a, meshes)
    ext = S.extent(a)
    ctx = _context(gpu_lib, blob)
    ids = [s.create(ctx) for s in sets]
    assert len(set(ids)) == len(ids) and min(ids) >= 16
    sid = ctx.create_skin(skin.first, skin.rest, skin.indices, skin.weights, skin.bones_count) if path in ("pose_skins", "pose") else None
    mid = ctx.create_morph(ms.first, ms.count, ms.base, ms.targets) if path == "pose" else None
    assert np.array_equal(bits(ctx.read_accel(4)), bits(a.vertices))  # (creating a set writes nothing)

    def write(seed, state):
        """one call of `path`; the vertex array it leaves BEFORE the recompute, by the host builds"""
        if path == "update_vertices":
            v = NC.posed(a, meshes, seed)
            assert ctx.update_vertices(0, v) == 0
            return v
        if path == "update_vertices_device":
            v = NC.posed(a, meshes, seed)
            t = _on_device(v)
            assert ctx.update_vertices_device(0, len(v), t.data_ptr()) == 0
            return v
        palette = S.palette(skin.bones_count, 40 + seed, ext)
        if path == "pose_skins":
            assert ctx.pose_skins({sid: palette}) == 0
            return S.host_posed(a, [skin], [palette], vertices=state)
        w = np.array([1.5, -0.5], dtype=np.float32) if seed % 2 else np.array([0.75, 1.0], dtype=np.float32)
        assert ctx.pose({mid: w}, {sid: palette}) == 0
        return M.host_morphed(a, [ms], [w], [skin], [palette], vertices=state)

    state = _recomputed(a, tris, write(1, a.vertices), sets)
    got = ctx.read_accel(4)
    assert got.dtype == hip.VERTEX_DTYPE and np.array_equal(bits(got), bits(state))
    assert not np.array_equal(bits(got["n"]), bits(a.vertices["n"])) and not np.array_equal(bits(got["b"]), bits(a.vertices["b"]))
    # one set destroyed, another created afterwards: the next call recomputes what is live then, and nothing of the destroyed set's
    assert ctx.destroy_normals(ids[1]) == 0 and ctx.destroy_normals(ids[1]) == 2
    mirror = meshes["mirror"]
    sets = [s for k, s in enumerate(sets) if k != 1] + [Set(a, mirror.first, mirror.count, N | B, weld=True)]
    new_id = sets[-1].create(ctx)
    assert new_id >= 16 and new_id not in ids
    state = _recomputed(a, tris, write(2, state), sets)
    assert np.array_equal(bits(ctx.read_accel(4)), bits(state))


def test_a_bitangent_set_at_the_upload_pose_reproduces_the_scene_builds_bitangents(gpu_lib, cloth):
    """the device against the reference's own bitangents: one set over the two sheets, twins and fallback faces included"""
    blob, a, meshes, _ = cloth
    sheet, mirror = meshes["sheet"], meshes["mirror"]
    assert mirror.first == sheet.first + sheet.count
    ctx = _context(gpu_lib, blob)
    assert ctx.create_normals(sheet.first, sheet.count + mirror.count, normals=False, bitangents=True) >= 16
    assert ctx.update_vertices(0, a.vertices) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(a.vertices))
    zeroed = a.vertices.copy()
    zeroed["b"][sheet.first:mirror.first + mirror.count] = 0.0  # (whatever arrives in b: it is not read)
    assert ctx.update_vertices(0, zeroed) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(a.vertices))


def test_arrays_and_frames_equal_a_host_built_update(gpu_lib, cloth):
    """... and an instance update keeps the sets.  The mirrored sheet's normal-mapped material reads the per-triangle bitangent table."""
    blob, a, meshes, tris = cloth
    sets = [Set(a, meshes[name].first, meshes[name].count, N | B, weld=name != "sheet") for name in ("sheet", "mirror", "fan", "sphere")]
    ctx, other, stale = _context(gpu_lib, blob), _context(gpu_lib, blob), _context(gpu_lib, blob)
    for s in sets:
        assert s.create(ctx) >= 16
    v = NC.posed(a, meshes, 1)
    want = _recomputed(a, tris, v, sets)
    assert ctx.update_vertices(0, v) == 0 and other.update_vertices(0, want) == 0 and stale.update_vertices(0, v) == 0
    assert _same(_accel(ctx), _accel(other)) and np.array_equal(ctx.read_accel(3), other.read_accel(3))
    frames = _frames(ctx)
    assert np.array_equal(frames, _frames(other))
    assert not np.array_equal(frames, _frames(stale))  # (the frames read n and b: with the uploaded ones they are other frames)
    moved = S.moved_blob(blob, a, want, 2, (0.01, 0.0, -0.01))
    assert ctx.update_instances(moved) == 0 and other.update_instances(moved) == 0
    v = NC.posed(a, meshes, 2)
    want = _recomputed(a, tris, v, sets)
    assert ctx.update_vertices(0, v) == 0 and other.update_vertices(0, want) == 0
    assert _same(_accel(ctx), _accel(other)) and np.array_equal(_frames(ctx), _frames(other))


def test_refusals_and_return_codes(gpu_lib, cloth, monkeypatch):
    blob, a, meshes, tris = cloth
    sheet, fan = meshes["sheet"], meshes["fan"]
    create, destroy = gpu_lib.fn("normals_create"), gpu_lib.fn("normals_destroy")
    empty = _context(gpu_lib)  # nothing uploaded yet
    assert empty.create_normals(0, 8) == 2 and empty.destroy_normals(16) == 2
    ctx = _context(gpu_lib, blob)
    first = ctx.create_normals(sheet.first + 5, 100)
    assert first >= 16
    with pytest.raises(RuntimeError, match="overlap"):
        ctx.create_normals(sheet.first + 104, 8)
    with pytest.raises(RuntimeError, match="outside"):
        ctx.create_normals(len(a.vertices) - 7, 8)
    with pytest.raises(RuntimeError, match="outside"):
        ctx.create_normals(fan.first, 0)
    with pytest.raises(RuntimeError, match="flags"):
        ctx.create_normals(fan.first, 8, normals=False, bitangents=False)
    out = hip.C.c_int(-1)
    d = hip.NormalsDesc(fan.first, 8, 4, None)
    assert create(ctx._ctx, hip.C.byref(d), hip.C.byref(out)) == 1 and b"flags" in gpu_lib.fn("last_error")()
    d = hip.NormalsDesc(fan.first, 8, 3, None)
    assert create(ctx._ctx, None, hip.C.byref(out)) == 1 and create(ctx._ctx, hip.C.byref(d), None) == 1 and create(None, hip.C.byref(d), hip.C.byref(out)) == 1
    assert out.value == -1
    weld = np.arange(8, dtype=np.uint32)
    weld[3] = 8
    with pytest.raises(RuntimeError, match="outside the range"):
        ctx.create_normals(fan.first, 8, weld=weld)
    weld[3], weld[2] = 2, 1  # (3 -> 2 -> 1: not canonical)
    with pytest.raises(RuntimeError, match="not canonical"):
        ctx.create_normals(fan.first, 8, weld=weld)
    assert ctx.destroy_normals(first + 1) == 2 and ctx.destroy_normals(5) == 2 and ctx.destroy_normals(0) == 2
    lights = a.light_vertices()
    assert ctx.create_normals(lights[0], 2) == 2  # the switch is off: the skins' rule
    assert np.array_equal(bits(ctx.read_accel(4)), bits(a.vertices))
    # sixteen sets are live at most; handles are distinct and never reused; an upload discards them all
    many = [first] + [ctx.create_normals(fan.first + k, 1) for k in range(15)]
    assert len(set(many)) == 16 and min(many) >= 16
    with pytest.raises(RuntimeError, match="live already"):
        ctx.create_normals(fan.first + 15, 1)
    assert ctx.destroy_normals(many[7]) == 0
    again = ctx.create_normals(fan.first + 6, 1)  # (many[7] covered it)
    assert again >= 16 and again not in many
    assert np.array_equal(bits(ctx.read_accel(4)), bits(a.vertices))
    ctx.upload_scene_blob(blob)
    assert ctx.destroy_normals(again) == 2 and ctx.destroy_normals(first) == 2
    v = NC.posed(a, meshes, 1)
    assert ctx.update_vertices(0, v) == 0 and np.array_equal(bits(ctx.read_accel(4)), bits(v))  # no set: the records as they came
    later = ctx.create_normals(sheet.first + 5, 100)
    assert later >= 16 and later not in many and later != again
    assert ctx.update_vertices(0, v) == 0
    assert np.array_equal(bits(ctx.read_accel(4)), bits(NC.host_recompute(a, v, tris, sheet.first + 5, 100, N | B)))
    # the 8-wide tree is built on the host only
    monkeypatch.setenv("RAYHIP_BVH_WIDTH", "8")
    wide = _context(gpu_lib, blob)
    monkeypatch.delenv("RAYHIP_BVH_WIDTH")
    assert wide.bvh_width() == 8
    assert wide.create_normals(fan.first, 8) == 2 and wide.destroy_normals(16) == 2
    assert np.array_equal(bits(wide.read_accel(4)), bits(a.vertices))


def test_a_set_over_the_rooms_emissive_quad(gpu_lib, cloth):
    blob, a, meshes, tris = cloth
    room = meshes["room"]
    lights = a.light_vertices()
    assert lights and set(lights) <= set(range(room.first, room.first + room.count))
    off = _context(gpu_lib, blob)
    assert off.create_normals(room.first, room.count) == 2 and np.array_equal(bits(off.read_accel(4)), bits(a.vertices))
    ctx, other = _context(gpu_lib, blob, refit=True), _context(gpu_lib, blob, refit=True)
    nid = ctx.create_normals(room.first, room.count)
    assert nid >= 16
    v = NC.posed(a, meshes, 1, names=("room", "sheet"), amplitude=0.004)
    assert not np.array_equal(bits(v["p"][lights]), bits(a.vertices["p"][lights]))
    want = NC.host_recompute(a, v, tris, room.first, room.count, N | B)
    assert ctx.update_vertices(0, v) == 0 and other.update_vertices(0, want) == 0
    kinds = (0, 1, 2, 4, 5, 6, 7)
    assert _same(_accel(ctx, kinds), _accel(other, kinds))
    assert np.array_equal(_frames(ctx), _frames(other))
    with pytest.raises(RuntimeError, match="covers vertex"):
        ctx.refit_lights(False)
    assert ctx.destroy_normals(nid) == 0 and ctx.refit_lights(False) == 0


def test_the_trace_of_an_update_without_a_set_is_what_it_was(gpu_lib, cloth, monkeypatch, capfd):
    blob, a, meshes, _ = cloth
    ctx = _context(gpu_lib, blob)
    v = NC.posed(a, meshes, 1)

    def traced():
        capfd.readouterr()
        monkeypatch.setenv("RAYHIP_TRACE_UPLOAD", "1")
        assert ctx.update_vertices(0, v) == 0
        monkeypatch.delenv("RAYHIP_TRACE_UPLOAD")
        lines = [line for line in capfd.readouterr().err.splitlines() if line.startswith("rayhip_scene_update_vertices")]
        return [line.split(" ms  ")[-1] if " ms  " in line else line for line in lines]  # (without the times)

    before = traced()
    assert before == ["begin", "vertices copied", "triangle records", "boxes refitted", "tri_verts done", "bvh4 built",
                      "rayhip_scene_update_vertices: 0 triangles without area", "top level built"]
    nid = ctx.create_normals(meshes["fan"].first, meshes["fan"].count)
    during = traced()
    assert during == before[:2] + ["normals recomputed"] + before[2:]
    assert ctx.destroy_normals(nid) == 0 and traced() == before
