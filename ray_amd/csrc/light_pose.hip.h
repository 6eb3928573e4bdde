// light_pose.hip.h -- the device side of moving and recolouring analytic lights (rayhip_scene_set_lights[_device]; rayhip_deform.hip.h):
// the element functions of light_pose.h.  k_pose_lights only READS what a render pass reads: the new records and their summaries go to
// a staging array and the findings to counters, so a refused call has touched nothing; k_commit_lights runs once the counters came
// back zero, and the level launches of light_refit.hip.h refit the tree behind it.  Both kernels are tiny (130 lights: one block):
// the call is bound by its launches and its read-back, not by them.
#pragma once

#include <hip/hip_runtime.h>

#include "light_pose.h"

namespace rayhip_light_pose {

// `flag` of every lane of the wavefront counted into *counter by ONE vector atomic: every lane of the block must get here (a wave64
// ballot; lane 0 of each wavefront adds the population count)
__device__ __forceinline__ void count_wave(const bool flag, uint32_t *counter) {
    const unsigned long long mask = __ballot(flag);
    if ((threadIdx.x & 63u) == 0u && mask != 0ull) {
        atomicAdd(counter, uint32_t(__popcll(mask)));
    }
}

__device__ __forceinline__ rayhip_light light_of_rows(const float4 r0, const float4 r1, const float4 r2, const float4 r3) {
    rayhip_light l;
    l.flags = __float_as_uint(r0.x), l.col[0] = r0.y, l.col[1] = r0.z, l.col[2] = r0.w;
    l.params[0] = r1.x, l.params[1] = r1.y, l.params[2] = r1.z, l.params[3] = r1.w, l.params[4] = r2.x, l.params[5] = r2.y, l.params[6] = r2.z, l.params[7] = r2.w;
    l.params[8] = r3.x, l.params[9] = r3.y, l.params[10] = r3.z, l.params[11] = r3.w;
    return l;
}

// a record of a 16-byte-aligned array as four 16-byte loads
__device__ __forceinline__ rayhip_light load_light16(const rayhip_light *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    return light_of_rows(q[0], q[1], q[2], q[3]);
}

// one lane per named entry: slot and record in (`aligned16`: `records` is 16-byte aligned; otherwise sixteen 4-byte loads), checked
// against the record the slot holds (`lights`, read only) and against `live` (one byte per slot: li_indices names it); `claim`: one word
// per slot, zero when the kernel starts -- the second lane to name a slot finds the first one's mark.  Out into the staging arrays:
// the record as four float4, its summary as three (staged_leaf: 48-byte records in a 16-byte-aligned array), the slot.
// counters[N_FINDINGS].
__global__ void __launch_bounds__(256) k_pose_lights(const uint32_t *__restrict__ slots, const rayhip_light *__restrict__ records, const uint32_t n,
                                                    const bool aligned16, const rayhip_light *__restrict__ lights, const uint32_t n_lights,
                                                    const uint8_t *__restrict__ live, uint32_t *__restrict__ claim, float4 *__restrict__ staged,
                                                    float4 *__restrict__ staged_leaf, uint32_t *__restrict__ staged_slots, uint32_t *__restrict__ counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n;
    bool is_bad_slot = false, duplicate = false, is_bad_type = false, is_changed = false, not_finite = false;
    if (active) {
        const uint32_t slot = slots[i];
        rayhip_light l;
        if (aligned16) {
            l = load_light16(records + i);
        } else {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(records) + size_t(i) * 16;
            l.flags = w[0];
            for (int k = 0; k < 3; ++k) {
                l.col[k] = __uint_as_float(w[1 + k]);
            }
            for (int k = 0; k < 12; ++k) {
                l.params[k] = __uint_as_float(w[4 + k]);
            }
        }
        not_finite = !finite_record(l);
        is_bad_slot = !slot_ok(slot, live, n_lights);
        if (!is_bad_slot) {
            duplicate = atomicAdd(&claim[slot], 1u) != 0u;
            const rayhip_light held = load_light16(lights + slot); // (the light array is the library's: 16-byte aligned)
            is_bad_type = bad_type(held, l), is_changed = flags_changed(held, l);
        }
        Summary s;
        analytic_light_summary(l, s);
        float4 *out = staged + size_t(i) * 4;
        out[0] = float4{__uint_as_float(l.flags), l.col[0], l.col[1], l.col[2]};
        out[1] = float4{l.params[0], l.params[1], l.params[2], l.params[3]};
        out[2] = float4{l.params[4], l.params[5], l.params[6], l.params[7]};
        out[3] = float4{l.params[8], l.params[9], l.params[10], l.params[11]};
        float4 *sum = staged_leaf + size_t(i) * 3;
        sum[0] = float4{s.lo[0], s.lo[1], s.lo[2], s.hi[0]};
        sum[1] = float4{s.hi[1], s.hi[2], s.flux, s.axis[0]};
        sum[2] = float4{s.axis[1], s.axis[2], s.omega_n, s.omega_e};
        staged_slots[i] = slot;
    }
    count_wave(is_bad_slot, &counters[BAD_SLOT]);
    count_wave(duplicate, &counters[DUPLICATE]);
    count_wave(is_bad_type, &counters[BAD_TYPE]);
    count_wave(is_changed, &counters[FLAGS_CHANGED]);
    count_wave(not_finite, &counters[NOT_FINITE]);
}

// one lane per named entry, after the counters came back zero (every staged slot is inside the array and named once): the record into
// `lights`, the summary into the leaf table of the light refit, the slot's byte of `posed` set
__global__ void __launch_bounds__(256) k_commit_lights(const float4 *__restrict__ staged, const float4 *__restrict__ staged_leaf,
                                                      const uint32_t *__restrict__ staged_slots, const uint32_t n, rayhip_light *__restrict__ lights,
                                                      Summary *__restrict__ leaf, uint8_t *__restrict__ posed, const uint32_t n_lights) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t slot = staged_slots[i];
    if (slot >= n_lights) { // (checked already: never followed unchecked)
        return;
    }
    const float4 *in = staged + size_t(i) * 4;
    float4 *out = reinterpret_cast<float4 *>(lights + slot);
    out[0] = in[0], out[1] = in[1], out[2] = in[2], out[3] = in[3];
    const float4 *sum = staged_leaf + size_t(i) * 3;
    float4 *to = reinterpret_cast<float4 *>(leaf + slot);
    to[0] = sum[0], to[1] = sum[1], to[2] = sum[2];
    posed[slot] = 1;
}

} // namespace rayhip_light_pose
