"""Which calls the host side of scene deformation makes, and in which words it refuses: one fixed script, one process, plain text.

Every entry point of ray_amd/csrc/rayhip_deform.hip.h is called at least once on its accepting path and once per distinct refusal, with
RAYHIP_TRACE_UPLOAD set.  After each call: a `== name` line, the phase stamps the library wrote to the C stderr during the call (the
millisecond figures replaced by X), the return code and rayhip_last_error().  The text depends on the order of the synchronising HIP calls
inside each entry point (every stamp is one), on every return code and on every error text, and on nothing that varies from run to run:
tests/golden/deform_trace.txt holds it as the library wrote it BEFORE its host side was consolidated, and
tests/test_gpu_deform_trace.py compares.

Scenes: tests/golden's cornell_instances (128 vertices, the four of its triangle light are 20..23, seven live instances) and, for the
analytic lights it lacks, cornell_lights of tests/light_pose_cases.py.  Every refusal is one the library makes on the host or from a
counter its checking kernel wrote: nothing here faults.

usage: python tools/deform_trace.py > trace.txt
"""
import ctypes as C
import os
import re
import sys
import tempfile

import numpy as np
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import instance_pose_cases as IP  # noqa: E402
import light_pose_cases as P  # noqa: E402
import light_refit_cases as L  # noqa: E402
import morph_cases as M  # noqa: E402
import skin_cases as S  # noqa: E402
import util  # noqa: E402
import vertex_update_cases as V  # noqa: E402
from ray_amd import hip  # noqa: E402

os.environ["RAYHIP_TRACE_UPLOAD"] = "1"
LIB = None


def call(name, fn):
    """fn() with the C stderr caught; prints the marker, the stamps, the return code (1 where the wrapper raised) and the error text"""
    sys.stdout.flush()
    sys.stderr.flush()
    keep = os.dup(2)
    out = None
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
            rc = out if isinstance(out, int) and out in (0, 1, 2) else 0  # (a handle is 16 or more)
        except RuntimeError:
            rc = 1
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        log = f.read().decode(errors="replace")
    print("==", name)
    for line in log.splitlines():
        print(re.sub(r"\s+[0-9.]+ ms\b", " X ms", line))
    print("rc", rc)
    print("last_error:", LIB.fn("last_error")().decode())
    return out


def on_device(array):
    t = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def context(blob=None, refit=False):
    ctx = hip.Context(0, LIB)
    ctx.upload_static(util.pmj())
    ctx.resize(64, 64)
    if refit:
        ctx.refit_lights(True)
    if blob is not None:
        call("upload", lambda: ctx.upload_scene_blob(blob) and 0)
    return ctx


def create_skin(ctx, a, first, count, seed=1):
    s = S.Skin(a, first, count, 3, seed)
    return lambda: ctx.create_skin(first, None, s.indices, s.weights, 3)


ONE_TARGET = [(np.array([0], dtype=np.uint32), np.array([[0.01, 0.0, 0.0]], dtype=np.float32), None, None)]


def handles(name, create, destroy, ctx, a, live, clear, singles, light):
    """create: ok (`live`, returned), overlap, outside, the 17th live handle, a pinned vertex; destroy: ok and a stale handle.
    `create(first, count)` makes the call; `clear`: a range that meets nothing live; `singles`: 16 free vertices; `light`: a range over the light"""
    kept = call(f"{name}_create ok", create(*live))
    call(f"{name}_create overlap", create(live[0] + 2, 4))
    call(f"{name}_create outside", create(len(a.vertices) - 3, 8))
    call(f"{name}_create empty range", create(clear[0], 0))
    call(f"{name}_create pinned", create(*light))
    many = [call(f"{name}_create single {v}", create(v, 1)) for v in singles[:15]]
    call(f"{name}_create the 17th", create(singles[15], 1))
    call(f"{name}_create overlap while full", create(singles[3], 1))
    for h in many:
        call(f"{name}_destroy {h}", lambda: destroy(h))
    call(f"{name}_destroy stale", lambda: destroy(many[0]))
    again = call(f"{name}_create in the lowest free slot", create(*clear))
    call(f"{name}_destroy", lambda: destroy(again))
    call(f"{name}_destroy twice", lambda: destroy(again))
    call(f"{name}_destroy nothing", lambda: destroy(0))
    print("handles", kept, many, again)
    return kept


def slot_calls(name, host, device, n_slots, slots, records, bad):
    """the host and the device form of a slots-and-records call: ok, n == 0, a null pointer, a slot outside, a duplicate, and the
    refusals of `bad` ({name: (slots, records)})"""
    for form in ("host", "device"):
        def go(s, r):
            s, r = np.ascontiguousarray(s, dtype=np.uint32), np.ascontiguousarray(r)
            if form == "host":
                return lambda: host(s, r)
            ts, tr = on_device(s), on_device(r)
            return lambda: (device(len(s), ts.data_ptr() if len(s) else 0, tr.data_ptr() if len(s) else 0), ts, tr)[0]
        call(f"{name} {form}: ok", go(slots, records))
        call(f"{name} {form}: ok again, one entry", go(slots[:1], records[:1]))
        call(f"{name} {form}: n == 0", go(slots[:0], records[:0]))
        outside = slots.copy()
        outside[-1] = n_slots
        call(f"{name} {form}: bad slot", go(outside, records))
        twice = slots.copy()
        twice[-1] = twice[0]
        call(f"{name} {form}: duplicate", go(twice, records))
        for what, (s, r) in bad.items():
            call(f"{name} {form}: {what}", go(s, r))
    call(f"{name} device: a null pointer", lambda: device(3, 0, 0))


def main():
    global LIB
    LIB = hip.Library()
    if LIB.device_count() <= 0:
        sys.exit("deform_trace needs a GPU")
    blob = util.golden_scene("cornell_instances")
    a = L.Arrays(blob)
    lights = a.light_vertices()
    assert len(a.vertices) == 128 and lights == [20, 21, 22, 23]
    ctx = context(blob)
    nan = np.float32(np.nan)

    # ---- vertex updates
    moved = V.perturbed_vertices(a, seed=7, fraction=0.02)
    used = [int(v) for v in S.used_vertices(a) if v not in lights]
    call("update_vertices ok", lambda: ctx.update_vertices(0, moved))
    call("update_vertices part", lambda: ctx.update_vertices(30, a.vertices[30:77]))
    call("update_vertices empty", lambda: ctx.update_vertices(5, a.vertices[:0]))
    call("update_vertices outside", lambda: ctx.update_vertices(120, a.vertices[:20]))
    bad = a.vertices.copy()
    bad["p"][used[3], 1] = nan
    call("update_vertices not finite", lambda: ctx.update_vertices(0, bad))
    pinned = a.vertices.copy()
    pinned["p"][21, 1] += np.float32(0.01)
    call("update_vertices pinned", lambda: ctx.update_vertices(0, pinned))
    call("update_vertices_blob ok", lambda: ctx.update_vertices_blob(blob))
    for what, v in (("ok", moved), ("not finite", bad), ("a light vertex changed", pinned)):
        t = on_device(v)
        call(f"update_vertices_device {what}", lambda: ctx.update_vertices_device(0, len(v), t.data_ptr()))
    t = on_device(a.vertices)
    call("update_vertices_device outside", lambda: ctx.update_vertices_device(120, 20, t.data_ptr()))
    call("update_vertices_device empty", lambda: ctx.update_vertices_device(0, 0, 0))
    call("update_vertices_device back", lambda: ctx.update_vertices_device(0, len(a.vertices), t.data_ptr()))

    # ---- handles over vertex ranges: a skin over [24, 128), a morph set inside it, a normal set over [1, 20)
    def create_morph(first, count):
        targets = M.seeded_set(a, first, count, 3, 5).targets if count >= 8 else ONE_TARGET
        return lambda: ctx.create_morph(first, count, None, targets)

    singles = list(range(1, 17))
    skin = handles("skin", lambda f, n: create_skin(ctx, a, f, n), ctx.destroy_skin, ctx, a, (24, 104), (1, 10), singles, (20, 4))
    inside = handles("morph", create_morph, ctx.destroy_morph, ctx, a, (37, 30), (1, 10), singles, (20, 4))
    normals = handles("normals", lambda f, n: (lambda: ctx.create_normals(f, n)), ctx.destroy_normals, ctx, a, (1, 19), (24, 10), list(range(24, 40)), (20, 4))
    call("normals_create bad flags", lambda: ctx.create_normals(30, 8, False, False))

    # ---- poses
    ext = S.extent(a)
    palette, w3 = S.palette(3, 2, ext), M.seeded_weights(3, 1)
    call("pose_skins: the skin holds a morph set", lambda: ctx.pose_skins({skin: palette}))
    call("pose: the skin holds a morph set", lambda: ctx.pose({}, {skin: palette}))
    call("pose: the morph set lies inside a skin", lambda: ctx.pose({inside: w3}, {}))
    call("pose: morph inside skin", lambda: ctx.pose({inside: w3}, {skin: palette}))
    short = call("skin_create short", create_skin(ctx, a, 1, 10, seed=2))
    across = call("morph_create across", create_morph(8, 8))
    call("pose: straddling", lambda: ctx.pose({across: w3}, {short: palette}))
    call("morph_destroy across", lambda: ctx.destroy_morph(across))
    alone = call("morph_create alone", create_morph(12, 8))
    call("pose: morph alone", lambda: ctx.pose({alone: w3}, {}))
    call("pose: everything", lambda: ctx.pose({alone: w3, inside: w3}, {short: palette, skin: palette}))
    call("pose: empty", lambda: ctx.pose({}, {}))
    call("pose: a stale morph set", lambda: ctx.pose({across: w3}, {}))
    call("pose: a weight that is not finite", lambda: ctx.pose({alone: [1.0, nan, 0.0]}, {}))
    call("pose: no skins allowed past 16", lambda: ctx.L.fn("scene_pose")(ctx._ctx, 0, None, None, 17, None, None))
    call("pose_skins ok", lambda: ctx.pose_skins({short: palette}))
    call("pose_skins empty", lambda: ctx.pose_skins({}))
    call("pose_skins bad arguments", lambda: ctx.L.fn("scene_pose_skins")(ctx._ctx, -1, None, None))
    call("pose_skins a stale skin", lambda: ctx.pose_skins({short + 16: palette}))
    ids, ptrs = (C.c_int * 2)(short, short), (C.c_void_p * 2)(palette.ctypes.data, palette.ctypes.data)
    call("pose_skins named twice", lambda: ctx.L.fn("scene_pose_skins")(ctx._ctx, 2, ids, ptrs))
    call("pose: a skin named twice", lambda: ctx.L.fn("scene_pose")(ctx._ctx, 0, None, None, 2, ids, ptrs))
    ptrs[1] = None
    ids[1] = skin
    call("pose_skins no palette", lambda: ctx.L.fn("scene_pose_skins")(ctx._ctx, 2, ids, ptrs))
    nan_palette = palette.copy()
    nan_palette[1, 0, 3] = nan
    call("pose_skins not finite", lambda: ctx.pose_skins({short: nan_palette}))
    call("morph_destroy alone", lambda: ctx.destroy_morph(alone))
    call("morph_destroy inside", lambda: ctx.destroy_morph(inside))
    call("pose_skins both", lambda: ctx.pose_skins({skin: S.identity_palette(3), short: S.identity_palette(3)}))

    # ---- instances that move, the switch off: the slot of the lamp is pinned
    lamp = IP.light_slots(a)
    free = [s for s in a.live_instances() if s not in lamp]
    assert len(lamp) == 1 and len(free) == 6
    slots = np.array(free[:4], dtype=np.uint32)
    xforms = IP.gentle_xforms(a, slots, seed=3)
    singular = xforms.copy()
    singular[1] = 0.0
    with_lamp = np.array([free[0], lamp[0]], dtype=np.uint32)
    bad = {"singular": (slots, singular), "pinned": (with_lamp, IP.gentle_xforms(a, with_lamp, seed=4))}
    slot_calls("set_instance_transforms", ctx.set_instance_transforms, ctx.set_instance_transforms_device, len(a.mesh_instances), slots, xforms, bad)
    records = a.lights[a.tri_lights()[:1]]
    call("set_lights: the switch is off", lambda: ctx.set_lights(a.tri_lights()[:1], records))
    t = on_device(records)
    call("set_lights_device: the switch is off", lambda: ctx.set_lights_device(1, t.data_ptr(), t.data_ptr()))

    # ---- the switch
    call("refit_lights off while off", lambda: ctx.refit_lights(False))
    call("refit_lights on", lambda: ctx.refit_lights(True))
    call("refit_lights on while on", lambda: ctx.refit_lights(True))
    call("update_vertices moves the light", lambda: ctx.update_vertices(0, pinned))
    t = on_device(pinned)
    call("update_vertices_device moves the light", lambda: ctx.update_vertices_device(0, len(pinned), t.data_ptr()))
    call("set_instance_transforms moves the lamp", lambda: ctx.set_instance_transforms(*bad["pinned"]))
    call("set_lights: a triangle light", lambda: ctx.set_lights(a.tri_lights()[:1], records))
    over = {"skin": call("skin_create over the light", create_skin(ctx, a, 20, 4)),
            "morph": call("morph_create over the light", create_morph(20, 4)),
            "normals": call("normals_create over the light", lambda: ctx.create_normals(20, 4))}
    call("pose moves the light", lambda: ctx.pose({over["morph"]: [0.5]}, {over["skin"]: palette}))
    for what, destroy in (("skin", ctx.destroy_skin), ("morph", ctx.destroy_morph), ("normals", ctx.destroy_normals)):
        call(f"refit_lights off under a {what}", lambda: ctx.refit_lights(False))
        call(f"{what}_destroy over the light", lambda: destroy(over[what]))
    call("refit_lights off", lambda: ctx.refit_lights(False))
    call("update_vertices pinned again", lambda: ctx.update_vertices(0, a.vertices))
    call("skin_create pinned again", create_skin(ctx, a, 20, 4))
    call("normals_destroy", lambda: ctx.destroy_normals(normals))
    call("upload again", lambda: ctx.upload_scene_blob(blob) and 0)
    call("skin_destroy after the upload", lambda: ctx.destroy_skin(skin))
    call("skin_create after the upload", create_skin(ctx, a, 24, 104))
    ctx.close()

    # ---- analytic lights that move
    lit = P.cornell_blob()
    la, lmoved = L.Arrays(lit), L.Arrays(P.cornell_blob(P.KINDS))
    slot_of = P.cornell_slots(la)
    slots = np.array([slot_of[k] for k in P.KINDS], dtype=np.uint32)
    records = lmoved.lights[slots].copy()
    flags, not_finite = records.copy(), records.copy()
    flags[2, 0] ^= 1 << 4
    not_finite[3, 9] = nan.view(np.uint32)
    tri = records.copy()
    tri[1, 0] = (tri[1, 0] & ~np.uint32(7)) | P.TYPE_TRI
    ctx = context(lit, refit=True)
    slot_calls("set_lights", ctx.set_lights, ctx.set_lights_device, len(la.lights), slots, records,
               {"a triangle light": (slots, tri), "word 0 changed": (slots, flags), "not finite": (slots, not_finite)})
    call("update_vertices behind posed lights", lambda: ctx.update_vertices(0, la.vertices))
    ctx.close()

    # ---- contexts that cannot: nothing uploaded, and the 8-wide tree
    def refusals(name, ctx, with_lights):
        call(f"{name}: update_vertices", lambda: ctx.update_vertices(0, a.vertices))
        t = on_device(a.vertices)
        call(f"{name}: update_vertices_device", lambda: ctx.update_vertices_device(0, len(a.vertices), t.data_ptr()))
        call(f"{name}: skin_create", create_skin(ctx, a, 24, 104))
        call(f"{name}: morph_create", lambda: ctx.create_morph(30, 1, None, ONE_TARGET))
        call(f"{name}: normals_create", lambda: ctx.create_normals(30, 8))
        call(f"{name}: pose_skins", lambda: ctx.pose_skins({16: palette}))
        call(f"{name}: pose_skins empty", lambda: ctx.pose_skins({}))
        call(f"{name}: pose", lambda: ctx.pose({16: w3}, {}))
        call(f"{name}: pose empty", lambda: ctx.pose({}, {}))
        call(f"{name}: set_instance_transforms", lambda: ctx.set_instance_transforms(free[:4], xforms))
        call(f"{name}: set_instance_transforms n == 0", lambda: ctx.set_instance_transforms(free[:0], xforms[:0]))
        call(f"{name}: set_instance_transforms_device null", lambda: ctx.set_instance_transforms_device(2, 0, 0))
        if with_lights:
            call(f"{name}: set_lights", lambda: ctx.set_lights(a.tri_lights()[:1], a.lights[a.tri_lights()[:1]]))
            call(f"{name}: set_lights n == 0", lambda: ctx.set_lights(slots[:0], records[:0]))

    none = hip.Context(0, LIB)
    call("no scene: refit_lights on", lambda: none.refit_lights(True))
    refusals("no scene", none, True)
    none.close()
    os.environ["RAYHIP_BVH_WIDTH"] = "8"
    wide = context(blob)
    del os.environ["RAYHIP_BVH_WIDTH"]
    assert wide.bvh_width() == 8
    refusals("8-wide", wide, False)
    wide.close()


if __name__ == "__main__":
    main()
