"""Cases of moving instances on the device (rayhip_scene_set_instance_transforms; ray_amd/csrc/instances.h): the host build of the
element functions (tests/hostsim/hostsim_instances.cpp), an independent numpy restatement of the inverse, seeded transform sets, and
the scene a context holds after a call, as a blob.  Shared by tests/test_instance_pose_hostsim.py and tests/test_gpu_instance_pose.py."""
import ctypes as C
import os

import numpy as np

import util
import vertex_update_cases as V

INSTANCES_LIB = os.path.join(util.ROOT, "tests", "hostsim", "_build", "libhostsim_instances.so")
SLOT_LIVE, SLOT_TRI_LIGHTS = 1, 2  # instances.h
BAD_SLOT, DUPLICATE, NOT_FINITE, PINNED = 0, 1, 2, 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the host build -------------------------------------------------------------------------------------------------------------
_lib = None


def instances_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(INSTANCES_LIB)
        vp, u32 = C.c_void_p, C.c_uint32
        _lib.hostsim_inverse_matrices.argtypes = [vp, u32, vp]
        _lib.hostsim_finite16.argtypes = [vp]
        _lib.hostsim_world_boxes.argtypes = [vp, u32, vp, u32, vp, u32, vp]
        _lib.hostsim_pose_instances.argtypes = [vp, u32, vp, C.c_int, u32, vp, vp, vp]
    return _lib


def host_inverse(xforms):
    """[n][16] float32: the inverses by tests/hostsim/hostsim_instances.cpp"""
    xforms = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1, 16)
    out = np.zeros_like(xforms)
    with np.errstate(all="ignore"):
        assert instances_lib().hostsim_inverse_matrices(xforms.ctypes.data, len(xforms), out.ctypes.data) == 0
    return out


def host_finite16(m):
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(16)
    return bool(instances_lib().hostsim_finite16(m.ctypes.data))


def host_world_boxes(nodes, mesh_instances, slots):
    """[n][6] f32 (lo, hi): the box of each slot's tree root under its transform"""
    nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
    mesh_instances = np.ascontiguousarray(mesh_instances, dtype=V.MESH_INSTANCE_DTYPE)
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    out = np.zeros((len(slots), 6), dtype=np.float32)
    rc = instances_lib().hostsim_world_boxes(nodes.ctypes.data, len(nodes), mesh_instances.ctypes.data, len(mesh_instances), slots.ctypes.data, len(slots),
                                             out.ctypes.data)
    assert rc == 0
    return out


def slot_flags(a: V.Arrays):
    """one byte per slot of the instance array: SLOT_LIVE where the top level names it, SLOT_TRI_LIGHTS where a triangle light hangs on it"""
    flags = np.zeros(len(a.mesh_instances), dtype=np.uint8)
    flags[a.live_instances()] |= SLOT_LIVE
    for i in a.li_indices:
        if a.lights[i, 0] & 7 == V.LIGHT_TYPE_TRI:
            flags[int(a.lights[i, 5])] |= SLOT_TRI_LIGHTS  # params[1]: the instance, as bits
    return flags


def light_slots(a: V.Arrays):
    return [int(s) for s in np.nonzero(slot_flags(a) & SLOT_TRI_LIGHTS)[0]]


def host_pose(mesh_instances, flags, slots, xforms, pin_lights=True):
    """(return code, the instance array after the call, findings [4]) by tests/hostsim/hostsim_instances.cpp"""
    mi = np.ascontiguousarray(mesh_instances, dtype=V.MESH_INSTANCE_DTYPE).copy()
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    slots = np.ascontiguousarray(slots, dtype=np.uint32).ravel()
    xforms = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1, 16)
    assert len(slots) == len(xforms) and len(flags) == len(mi)
    findings = np.zeros(4, dtype=np.uint32)
    with np.errstate(all="ignore"):
        rc = instances_lib().hostsim_pose_instances(mi.ctypes.data, len(mi), flags.ctypes.data, 1 if pin_lights else 0, len(slots), slots.ctypes.data,
                                                    xforms.ctypes.data, findings.ctypes.data)
    return rc, mi, findings


def moved_instances(a: V.Arrays, slots, xforms, pin_lights=False):
    """the instance array of `a` after an accepted call"""
    rc, mi, findings = host_pose(a.mesh_instances, slot_flags(a), slots, xforms, pin_lights)
    assert rc == 0, (rc, findings)
    return mi


# ---- numpy restatement: float32, one rounding per operation, the order of the reference's InverseMatrix written out --------------------
def numpy_inverse(xforms):
    """[n][16] float32 inverses: internal/Core.cpp:1390-1431 operation for operation"""
    f = np.float32
    m = np.ascontiguousarray(xforms, dtype=f).reshape(-1, 16).T  # m[k]: element k of every matrix

    def minor(a, b, c, d):
        return m[a] * m[b] - m[c] * m[d]

    with np.errstate(all="ignore"):
        A2323, A1323, A1223 = minor(10, 15, 11, 14), minor(9, 15, 11, 13), minor(9, 14, 10, 13)
        A0323, A0223, A0123 = minor(8, 15, 11, 12), minor(8, 14, 10, 12), minor(8, 13, 9, 12)
        A2313, A1313, A1213 = minor(6, 15, 7, 14), minor(5, 15, 7, 13), minor(5, 14, 6, 13)
        A2312, A1312, A1212 = minor(6, 11, 7, 10), minor(5, 11, 7, 9), minor(5, 10, 6, 9)
        A0313, A0213, A0312 = minor(4, 15, 7, 12), minor(4, 14, 6, 12), minor(4, 11, 7, 8)
        A0212, A0113, A0112 = minor(4, 10, 6, 8), minor(4, 13, 5, 12), minor(4, 9, 5, 8)

        def cof(a, x, b, y, c, z):
            return m[a] * x - m[b] * y + m[c] * z

        det = m[0] * cof(5, A2323, 6, A1323, 7, A1223) - m[1] * cof(4, A2323, 6, A0323, 7, A0223) + m[2] * cof(4, A1323, 5, A0323, 7, A0123) - \
            m[3] * cof(4, A1223, 5, A0223, 6, A0123)
        inv_det = f(1.0) / det
        assert det.dtype == f and inv_det.dtype == f
        out = [inv_det * cof(5, A2323, 6, A1323, 7, A1223), inv_det * -cof(1, A2323, 2, A1323, 3, A1223), inv_det * cof(1, A2313, 2, A1313, 3, A1213),
               inv_det * -cof(1, A2312, 2, A1312, 3, A1212), inv_det * -cof(4, A2323, 6, A0323, 7, A0223), inv_det * cof(0, A2323, 2, A0323, 3, A0223),
               inv_det * -cof(0, A2313, 2, A0313, 3, A0213), inv_det * cof(0, A2312, 2, A0312, 3, A0212), inv_det * cof(4, A1323, 5, A0323, 7, A0123),
               inv_det * -cof(0, A1323, 1, A0323, 3, A0123), inv_det * cof(0, A1313, 1, A0313, 3, A0113), inv_det * -cof(0, A1312, 1, A0312, 3, A0112),
               inv_det * -cof(4, A1223, 5, A0223, 6, A0123), inv_det * cof(0, A1223, 1, A0223, 2, A0123), inv_det * -cof(0, A1213, 1, A0213, 2, A0113),
               inv_det * cof(0, A1212, 1, A0212, 2, A0112)]
    out = np.stack(out, axis=-1)
    assert out.dtype == f
    return out


# ---- seeded transforms ------------------------------------------------------------------------------------------------------------
def identity():
    return np.eye(4, dtype=np.float32).ravel()


def seeded_xforms(n, seed, centre=(-0.28, 0.1, -0.28), spread=0.2, mirrored=False):
    """[n][16] float32 in the layout of rayhip_mesh_instance::xform (column vectors, translation in elements 12..14): rotation about a
    random axis x non-uniform scale x shear, + a translation within `spread` of `centre`.  `mirrored`: one scale negative (det < 0)."""
    rng = np.random.RandomState(seed)
    out = np.zeros((n, 16), dtype=np.float32)
    for i in range(n):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = rng.uniform(-np.pi, np.pi)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
        S = np.diag(rng.uniform(0.4, 1.6, size=3))
        if mirrored:
            S[rng.randint(0, 3), :] *= -1.0
        H = np.eye(3)
        H[0, 1], H[0, 2], H[1, 2] = rng.uniform(-0.3, 0.3, size=3)
        m = np.eye(4)
        m[:3, :3] = R @ S @ H
        m[:3, 3] = np.asarray(centre) + rng.uniform(-spread, spread, size=3)
        out[i] = m.T.astype(np.float32).ravel()
    return out


def gentle_xforms(a: V.Arrays, slots, seed, shift=0.04, turn_deg=12.0):
    """[n][16]: the transforms of `slots` in place, each turned about the y axis by up to `turn_deg` and shifted by up to `shift` in x and z -- a scene
    that still looks like itself (its instances stay inside the room)"""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(slots), 16), dtype=np.float32)
    for k, s in enumerate(slots):
        m = a.mesh_instances["xform"][s].astype(np.float64).reshape(4, 4).T  # column vectors
        t = np.radians(rng.uniform(-turn_deg, turn_deg))
        d = np.eye(4)
        d[0, 0], d[0, 2], d[2, 0], d[2, 2] = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
        d[0, 3], d[2, 3] = rng.uniform(-shift, shift, size=2)
        out[k] = (d @ m).T.astype(np.float32).ravel()
    return out


# ---- the scene after a call, as a blob ----------------------------------------------------------------------------------------------
def patch_top_level(a: V.Arrays, nodes, boxes_of_slot):
    """`nodes` ([n][16] u32, a copy) with the leaves of a's top level set to boxes_of_slot[slot] and the inner boxes refitted over them"""
    f = nodes.view(np.float32)

    def refit(w):
        out = []
        for k, link in enumerate(a.nodes[w, 12:14]):
            b = boxes_of_slot[int(link & V.INDEX_BITS)] if link & V.COUNT_BITS else refit(int(link))
            f[w, [0, 2, 8, 1, 3, 9] if k == 0 else [4, 6, 10, 5, 7, 11]] = b  # (vertex_update_cases.child_box: lo.xyz, hi.xyz)
            out.append(b)
        return np.concatenate([np.minimum(out[0][:3], out[1][:3]), np.maximum(out[0][3:], out[1][3:])])

    if a.tlas_root != 0xffffffff:
        refit(a.tlas_root)
    return nodes


def moved_blob(blob, a: V.Arrays, slots, xforms, vertices=None):
    """the scene with new transforms for `slots`, as rayhip_scene_update_instances or a fresh upload wants it: the instance array with
    the new matrices and the restated inverses, and the leaves of the top level with the world boxes of the live instances
    (V.instance_boxes: tests/hostsim/hostsim_refit.cpp) -- under `vertices` where the meshes were deformed before.  Any number of slots."""
    mi = a.mesh_instances.copy()
    xforms = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1, 16)
    for s, m in zip(slots, xforms):
        mi["xform"][s] = m
        mi["inv_xform"][s] = numpy_inverse(m)[0]
    nodes = a.nodes.copy() if vertices is None else V.host_refit(a, vertices)[1]
    live = a.live_instances()
    boxes = V.instance_boxes(nodes, mi, live)
    patch_top_level(a, nodes, dict(zip(live, boxes)))
    return V.patched_blob(blob, mesh_instances=mi, nodes=nodes)


def leaves_of(a: V.Arrays, mesh_instances, nodes=None):
    """what read_accel(3) holds after a call: [live][7] u32 words (slot, lo.xyz, hi.xyz), by the host build"""
    live = a.live_instances()
    boxes = host_world_boxes(a.nodes if nodes is None else nodes, mesh_instances, live)
    out = np.zeros((len(live), 7), dtype=np.uint32)
    out[:, 0] = live
    out[:, 1:] = bits(boxes)
    return out
