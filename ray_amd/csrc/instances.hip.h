// instances.hip.h -- the device side of moving instances (rayhip_scene_set_instance_transforms[_device]; rayhip_deform.hip.h): the
// element functions of instances.h.  k_pose_instances only READS what a render pass reads: the new records go to a staging array and
// the findings to counters, so a refused call has touched nothing; k_commit_instances and k_instance_boxes run once the counters came
// back zero.  All three are tiny (1000 instances: four blocks): the call is bound by its launches and read-backs, not by them.
#pragma once

#include <hip/hip_runtime.h>

#include "instances.h"

namespace rayhip_instances {

// `flag` of every lane of the wavefront counted into *counter by ONE vector atomic: every lane of the block must get here (a wave64
// ballot; lane 0 of each wavefront adds the population count)
__device__ __forceinline__ void count_wave(const bool flag, uint32_t *counter) {
    const unsigned long long mask = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u && mask != 0ull) {
        atomicAdd(counter, uint32_t(__popcll(mask)));
    }
}

// one lane per named entry: slot and matrix in (`aligned16`: `xforms` is 16-byte aligned, the matrix comes as four float4), the inverse
// computed, the 128-byte record (xform, inv_xform) and the slot out into the staging arrays.  `flags`: one byte per slot of the instance
// array (SLOT_LIVE, SLOT_TRI_LIGHTS); `claim`: one word per slot, zero when the kernel starts -- the second lane to name a slot finds
// the first one's mark.  `instances` is read only (the transform in place of a slot that carries lights).  counters[N_FINDINGS].
__global__ void __launch_bounds__(256) k_pose_instances(const uint32_t *__restrict__ slots, const float *__restrict__ xforms, const uint32_t n, const bool aligned16,
                                                       const uint8_t *__restrict__ flags, uint32_t *__restrict__ claim,
                                                       const rayhip_mesh_instance *__restrict__ instances, const uint32_t n_instances, const bool pin_lights,
                                                       float4 *__restrict__ staged, uint32_t *__restrict__ staged_slots, uint32_t *__restrict__ counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    bool bad_slot = false, duplicate = false, not_finite = false, is_pinned = false;
    if (active) {
        const uint32_t slot = slots[i];
        float m[16], inv[16];
        if (aligned16) {
            const float4 *q = reinterpret_cast<const float4 *>(xforms) + size_t(i) * 4;
            const float4 r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3];
            m[0] = r0.x, m[1] = r0.y, m[2] = r0.z, m[3] = r0.w, m[4] = r1.x, m[5] = r1.y, m[6] = r1.z, m[7] = r1.w;
            m[8] = r2.x, m[9] = r2.y, m[10] = r2.z, m[11] = r2.w, m[12] = r3.x, m[13] = r3.y, m[14] = r3.z, m[15] = r3.w;
        } else {
            for (int k = 0; k < 16; ++k) {
                m[k] = xforms[size_t(i) * 16 + k];
            }
        }
        inverse_matrix(m, inv);
        not_finite = !(finite16(m) && finite16(inv));
        bad_slot = !slot_ok(slot, flags, n_instances);
        if (!bad_slot) {
            duplicate = atomicAdd(&claim[slot], 1u) != 0u;
            is_pinned = pinned(flags[slot], pin_lights, m, instances[slot].xform);
        }
        float4 *out = staged + size_t(i) * 8;
        out[0] = float4{m[0], m[1], m[2], m[3]}, out[1] = float4{m[4], m[5], m[6], m[7]};
        out[2] = float4{m[8], m[9], m[10], m[11]}, out[3] = float4{m[12], m[13], m[14], m[15]};
        out[4] = float4{inv[0], inv[1], inv[2], inv[3]}, out[5] = float4{inv[4], inv[5], inv[6], inv[7]};
        out[6] = float4{inv[8], inv[9], inv[10], inv[11]}, out[7] = float4{inv[12], inv[13], inv[14], inv[15]};
        staged_slots[i] = slot;
    }
    count_wave(bad_slot, &counters[BAD_SLOT]);
    count_wave(duplicate, &counters[DUPLICATE]);
    count_wave(not_finite, &counters[NOT_FINITE]);
    count_wave(is_pinned, &counters[PINNED]);
}

// one lane per named entry, after the counters came back zero (every staged slot is inside the array and named once): bytes 16..143 of
// the slot's 144-byte record, eight float4 (the array is 16-byte aligned and 144 = 9 x 16)
__global__ void __launch_bounds__(256) k_commit_instances(const float4 *__restrict__ staged, const uint32_t *__restrict__ staged_slots, const uint32_t n,
                                                         rayhip_mesh_instance *__restrict__ instances, const uint32_t n_instances) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t slot = staged_slots[i];
    if (slot >= n_instances) { // (checked already: never followed unchecked)
        return;
    }
    const float4 *in = staged + size_t(i) * 8;
    float4 *out = reinterpret_cast<float4 *>(instances + slot) + 1;
    for (int k = 0; k < 8; ++k) {
        out[k] = in[k];
    }
}

// one lane per live slot: its record, the root node of its bottom-level tree as it is on the device now (the three 16-byte rows of its
// 64 bytes that hold the child boxes), the world box as six floats (lo.xyz, hi.xyz).  A slot whose root lies outside the nodes gets the
// empty box.
__global__ void __launch_bounds__(256) k_instance_boxes(const uint32_t *__restrict__ live, const uint32_t n_live, const rayhip_mesh_instance *__restrict__ instances,
                                                       const uint32_t n_instances, const rayhip_bvh2_node *__restrict__ nodes, const uint32_t n_nodes,
                                                       float *__restrict__ boxes) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_live) {
        return;
    }
    rayhip_lbvh::Box b = rayhip_lbvh::empty_box();
    const uint32_t slot = live[k];
    if (slot < n_instances) {
        const float4 *rec = reinterpret_cast<const float4 *>(instances + slot);
        const float4 head = rec[0], r0 = rec[1], r1 = rec[2], r2 = rec[3], r3 = rec[4];
        const uint32_t node_index = __float_as_uint(head.y);
        if (node_index < n_nodes) {
            const float4 *q = reinterpret_cast<const float4 *>(nodes + node_index);
            const float4 d0 = q[0], d1 = q[1], d2 = q[2];
            rayhip_bvh2_node root = {};
            root.ch_data0[0] = d0.x, root.ch_data0[1] = d0.y, root.ch_data0[2] = d0.z, root.ch_data0[3] = d0.w;
            root.ch_data1[0] = d1.x, root.ch_data1[1] = d1.y, root.ch_data1[2] = d1.z, root.ch_data1[3] = d1.w;
            root.ch_data2[0] = d2.x, root.ch_data2[1] = d2.y, root.ch_data2[2] = d2.z, root.ch_data2[3] = d2.w;
            const float xform[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
            b = world_box(root, xform);
        }
    }
    float *out = boxes + size_t(k) * 6;
    out[0] = b.lo[0], out[1] = b.lo[1], out[2] = b.lo[2], out[3] = b.hi[0], out[4] = b.hi[1], out[5] = b.hi[2];
}

} // namespace rayhip_instances
