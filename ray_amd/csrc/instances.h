// instances.h -- moving whole mesh instances of the scene that is on the device (rayhip_scene_set_instance_transforms and its _device
// form): new transforms in, inverses and world-space boxes out.  Element functions shared by the device kernels (instances.hip.h) and
// a plain-loop host driver (tests/hostsim/hostsim_instances.cpp), like skin.h: IEEE operations in a STATED ORDER without contraction
// on both sides, so both produce the same bits.
//
//   inv_xform   the reference's InverseMatrix (internal/Core.cpp:1390-1431) operation for operation: the eighteen 2x2 minors
//               a*b - c*d, the determinant as m0*(..) - m1*(..) + m2*(..) - m3*(..) with every cofactor (p - q) + r,
//               inv_det = 1.0f / det, and sixteen products inv_det * cofactor, the odd ones inv_det * -(cofactor).  This is what
//               SceneBase::SetMeshInstanceTransform stores, bit for bit.
//   world box   the eight corners of the box of the root node of the slot's bottom-level tree through rt::transform_point, min / max
//               from an empty box on: the operations of rayhip_rebuild::transform_box(node_box(root), xform) (scene_rebuild.h), which
//               the vertex update uses -- ONE box arithmetic in the library, so "move then pose" and "pose then move" leave the same
//               leaves.  Deliberately not the reference's TransformBoundingBox (an ulp or two apart).
//
// A call names slots; it is refused as a whole (nothing on the device written) when a named slot is outside the instance array or
// not in the top level, is named twice, gets a matrix with an element that is not finite or whose inverse has one (a singular
// matrix: inv_det = inf), or carries triangle lights while the lights are not refitted and its transform would change.
#pragma once

#include <stdint.h>

#include "lbvh.h"
#include "rt_types.h"

namespace rayhip_instances {

constexpr uint32_t SLOT_LIVE = 1u;       // per-slot flags: the top level names the slot ...
constexpr uint32_t SLOT_TRI_LIGHTS = 2u; // ... some triangle light hangs on it (params[1] of a light of type TRI)
// the findings of a call, one counter each
enum { BAD_SLOT = 0, DUPLICATE = 1, NOT_FINITE = 2, PINNED = 3, N_FINDINGS = 4 };

RT_HD bool finite_f(const float x) { return fabsf(x) <= 3.402823466e+38f; } // (false for NaN)

RT_HD bool finite16(const float m[16]) {
    bool ok = true;
    for (int k = 0; k < 16; ++k) {
        ok = ok && finite_f(m[k]);
    }
    return ok;
}

RT_HD void inverse_matrix(const float mat[16], float out_mat[16]) {
    const float A2323 = mat[10] * mat[15] - mat[11] * mat[14];
    const float A1323 = mat[9] * mat[15] - mat[11] * mat[13];
    const float A1223 = mat[9] * mat[14] - mat[10] * mat[13];
    const float A0323 = mat[8] * mat[15] - mat[11] * mat[12];
    const float A0223 = mat[8] * mat[14] - mat[10] * mat[12];
    const float A0123 = mat[8] * mat[13] - mat[9] * mat[12];
    const float A2313 = mat[6] * mat[15] - mat[7] * mat[14];
    const float A1313 = mat[5] * mat[15] - mat[7] * mat[13];
    const float A1213 = mat[5] * mat[14] - mat[6] * mat[13];
    const float A2312 = mat[6] * mat[11] - mat[7] * mat[10];
    const float A1312 = mat[5] * mat[11] - mat[7] * mat[9];
    const float A1212 = mat[5] * mat[10] - mat[6] * mat[9];
    const float A0313 = mat[4] * mat[15] - mat[7] * mat[12];
    const float A0213 = mat[4] * mat[14] - mat[6] * mat[12];
    const float A0312 = mat[4] * mat[11] - mat[7] * mat[8];
    const float A0212 = mat[4] * mat[10] - mat[6] * mat[8];
    const float A0113 = mat[4] * mat[13] - mat[5] * mat[12];
    const float A0112 = mat[4] * mat[9] - mat[5] * mat[8];

    const float inv_det = 1.0f / (mat[0] * (mat[5] * A2323 - mat[6] * A1323 + mat[7] * A1223) - mat[1] * (mat[4] * A2323 - mat[6] * A0323 + mat[7] * A0223) +
                                  mat[2] * (mat[4] * A1323 - mat[5] * A0323 + mat[7] * A0123) - mat[3] * (mat[4] * A1223 - mat[5] * A0223 + mat[6] * A0123));

    out_mat[0] = inv_det * (mat[5] * A2323 - mat[6] * A1323 + mat[7] * A1223);
    out_mat[1] = inv_det * -(mat[1] * A2323 - mat[2] * A1323 + mat[3] * A1223);
    out_mat[2] = inv_det * (mat[1] * A2313 - mat[2] * A1313 + mat[3] * A1213);
    out_mat[3] = inv_det * -(mat[1] * A2312 - mat[2] * A1312 + mat[3] * A1212);
    out_mat[4] = inv_det * -(mat[4] * A2323 - mat[6] * A0323 + mat[7] * A0223);
    out_mat[5] = inv_det * (mat[0] * A2323 - mat[2] * A0323 + mat[3] * A0223);
    out_mat[6] = inv_det * -(mat[0] * A2313 - mat[2] * A0313 + mat[3] * A0213);
    out_mat[7] = inv_det * (mat[0] * A2312 - mat[2] * A0312 + mat[3] * A0212);
    out_mat[8] = inv_det * (mat[4] * A1323 - mat[5] * A0323 + mat[7] * A0123);
    out_mat[9] = inv_det * -(mat[0] * A1323 - mat[1] * A0323 + mat[3] * A0123);
    out_mat[10] = inv_det * (mat[0] * A1313 - mat[1] * A0313 + mat[3] * A0113);
    out_mat[11] = inv_det * -(mat[0] * A1312 - mat[1] * A0312 + mat[3] * A0112);
    out_mat[12] = inv_det * -(mat[4] * A1223 - mat[5] * A0223 + mat[6] * A0123);
    out_mat[13] = inv_det * (mat[0] * A1223 - mat[1] * A0223 + mat[2] * A0123);
    out_mat[14] = inv_det * -(mat[0] * A1213 - mat[1] * A0213 + mat[2] * A0113);
    out_mat[15] = inv_det * (mat[0] * A1212 - mat[1] * A0212 + mat[2] * A0112);
}

// the world-space box of a tree under `xform`, `root` being the tree's root node
RT_HD rayhip_lbvh::Box world_box(const rayhip_bvh2_node &root, const float *xform) {
    rayhip_lbvh::Box b;
    b.lo[0] = fminf(root.ch_data0[0], root.ch_data1[0]), b.hi[0] = fmaxf(root.ch_data0[1], root.ch_data1[1]);
    b.lo[1] = fminf(root.ch_data0[2], root.ch_data1[2]), b.hi[1] = fmaxf(root.ch_data0[3], root.ch_data1[3]);
    b.lo[2] = fminf(root.ch_data2[0], root.ch_data2[2]), b.hi[2] = fmaxf(root.ch_data2[1], root.ch_data2[3]);
    rayhip_lbvh::Box o = rayhip_lbvh::empty_box();
    for (int k = 0; k < 8; ++k) {
        const rt::f3 p = rt::transform_point(rt::f3{(k & 1) ? b.hi[0] : b.lo[0], (k & 2) ? b.hi[1] : b.lo[1], (k & 4) ? b.hi[2] : b.lo[2]}, xform);
        const float q[3] = {p.x, p.y, p.z};
        rayhip_lbvh::grow_point(o, q);
    }
    return o;
}

// bytewise comparison of two matrices (what memcmp says, as sixteen words)
RT_HD bool same_matrix(const float *x, const float *y) {
    const uint32_t *a = reinterpret_cast<const uint32_t *>(x), *b = reinterpret_cast<const uint32_t *>(y);
    bool same = true;
    for (int k = 0; k < 16; ++k) {
        same = same && a[k] == b[k];
    }
    return same;
}

// a slot a call may name: inside the instance array and in the top level
RT_HD bool slot_ok(const uint32_t slot, const uint8_t *flags, const uint32_t n_instances) { return slot < n_instances && (flags[slot] & SLOT_LIVE) != 0; }

// a slot (one a call may name) that must stay where it is: it carries triangle lights, the lights are not refitted (`pin_lights`), and
// `xform` is not the transform in place bytewise
RT_HD bool pinned(const uint32_t slot_flags, const bool pin_lights, const float *xform, const float *in_place) {
    return pin_lights && (slot_flags & SLOT_TRI_LIGHTS) != 0 && !same_matrix(xform, in_place);
}

// what the findings of a call mean: 0 = go on, 1 = a bad slot, a duplicate or a bad matrix, 2 = the lights would have to be rebuilt
RT_HD int verdict(const uint32_t findings[N_FINDINGS]) {
    return (findings[BAD_SLOT] | findings[DUPLICATE] | findings[NOT_FINITE]) != 0 ? 1 : findings[PINNED] != 0 ? 2 : 0;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the whole call as plain loops: `instances` [n_instances] in place, `flags` one byte per slot.  The findings are counted as the
// device counts them; the array is written only where verdict() is 0, which is returned.
inline int pose_instances_host(rayhip_mesh_instance *instances, const uint32_t n_instances, const uint8_t *flags, const bool pin_lights, const uint32_t n,
                               const uint32_t *slots, const float *xforms, uint32_t findings[N_FINDINGS]) {
    for (int k = 0; k < N_FINDINGS; ++k) {
        findings[k] = 0;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const float *m = xforms + size_t(i) * 16;
        float inv[16];
        inverse_matrix(m, inv);
        findings[NOT_FINITE] += finite16(m) && finite16(inv) ? 0u : 1u;
        if (!slot_ok(slots[i], flags, n_instances)) {
            findings[BAD_SLOT] += 1;
            continue;
        }
        for (uint32_t j = 0; j < i; ++j) {
            if (slots[j] == slots[i]) {
                findings[DUPLICATE] += 1;
                break;
            }
        }
        findings[PINNED] += pinned(flags[slots[i]], pin_lights, m, instances[slots[i]].xform) ? 1u : 0u;
    }
    const int rc = verdict(findings);
    for (uint32_t i = 0; rc == 0 && i < n; ++i) {
        rayhip_mesh_instance &mi = instances[slots[i]];
        const float *m = xforms + size_t(i) * 16;
        float inv[16];
        inverse_matrix(m, inv);
        for (int k = 0; k < 16; ++k) {
            mi.xform[k] = m[k], mi.inv_xform[k] = inv[k];
        }
    }
    return rc;
}

} // namespace rayhip_instances
