// materials.hip.h -- the device side of changing materials (rayhip_scene_set_materials[_device]; rayhip_deform.hip.h): the element
// functions of materials.h.  k_check_materials only READS what a render pass reads: the new records go to a staging array and the
// findings to counters, so a refused call has touched nothing; k_commit_materials runs once the counters came back clean;
// k_recolour_tri_lights follows when an emitter was named, and the light refit (light_refit.hip.h) behind it.  All three are tiny (130
// materials: one block): the call is bound by its launches and its read-back, not by them.
#pragma once

#include <hip/hip_runtime.h>

#include "light_pose.hip.h" // count_wave
#include "materials.h"

namespace rayhip_materials {

using rayhip_light_pose::count_wave;

// one lane per named entry.  A record is 19 dwords and 16-byte aligned only every fourth entry (and `records` itself only 4-byte
// aligned), so a wavefront loads its 64 x 19 dwords as consecutive dwords -- on the way they go to `staged` as they are -- and hands
// them round through LDS: lane l reads the dwords 19 l + k, an odd stride, which no two lanes of a bank share.  Each record is judged
// against the one the slot holds (`materials`, read only), the slot's flags and `claim`: one word per slot, zero when the kernel
// starts -- the second lane to name a slot finds the first one's mark, and k_recolour_tri_lights finds the emitters that were named.
// counters[N_COUNTERS].
__global__ void __launch_bounds__(256) k_check_materials(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ records, const uint32_t n,
                                                        const rayhip_material *__restrict__ materials, const uint32_t n_materials,
                                                        const uint8_t *__restrict__ flags, uint32_t *__restrict__ claim, const bool plain_ior,
                                                        const bool refittable, uint32_t *__restrict__ staged, uint32_t *__restrict__ staged_slots,
                                                        uint32_t *__restrict__ counters) {
    __shared__ uint32_t words[4][64 * RECORD_WORDS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t first = blockIdx.x * blockDim.x + wave * 64u; // the first entry of this wavefront
    const uint32_t count = first < n ? (n - first < 64u ? n - first : 64u) : 0u;
    const size_t base = size_t(first) * RECORD_WORDS;
    for (uint32_t j = lane; j < count * RECORD_WORDS; j += 64u) {
        const uint32_t w = records[base + j];
        words[wave][j] = w;
        staged[base + j] = w;
    }
    __syncthreads();
    Judgement j;
    if (lane < count) {
        const uint32_t i = first + lane;
        uint32_t r[RECORD_WORDS];
        for (uint32_t k = 0; k < RECORD_WORDS; ++k) {
            r[k] = words[wave][lane * RECORD_WORDS + k];
        }
        rayhip_material m;
        memcpy(&m, r, sizeof(m));
        const uint32_t slot = slots[i];
        staged_slots[i] = slot;
        if (slot_ok(slot, flags, n_materials)) {
            j = judge_record(m, materials[slot], flags[slot], atomicAdd(&claim[slot], 1u) != 0u, plain_ior, refittable);
        } else {
            j.bad_slot = true, j.not_finite = !finite_record(m);
        }
    }
    count_wave(j.bad_slot, &counters[BAD_SLOT]);
    count_wave(j.duplicate, &counters[DUPLICATE]);
    count_wave(j.changed, &counters[GRAPH_CHANGED]);
    count_wave(j.not_finite, &counters[NOT_FINITE]);
    count_wave(j.negative, &counters[NEGATIVE]);
    count_wave(j.refracting, &counters[REFRACTS]);
    count_wave(j.pinned, &counters[PINNED]);
    count_wave(j.emitter, &counters[EMITTERS_NAMED]);
}

// one lane per dword of the staged records, after the counters came back clean (every staged slot is inside the array and named once):
// dword k of entry i into dword k of material slot staged_slots[i]
__global__ void __launch_bounds__(256) k_commit_materials(const uint32_t *__restrict__ staged, const uint32_t *__restrict__ staged_slots, const uint32_t n,
                                                         uint32_t *__restrict__ materials, const uint32_t n_materials) {
    const size_t at = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (at >= size_t(n) * RECORD_WORDS) {
        return;
    }
    const uint32_t i = uint32_t(at / RECORD_WORDS), k = uint32_t(at - size_t(i) * RECORD_WORDS);
    const uint32_t slot = staged_slots[i];
    if (slot >= n_materials) { // (checked already: never followed unchecked)
        return;
    }
    materials[size_t(slot) * RECORD_WORDS + k] = staged[at];
}

// one lane per light slot, behind the commit: a triangle light whose emitter was named takes its colour from the record that is in the
// material array now (`light_emitter`: materials.h, emitter_tables)
__global__ void __launch_bounds__(256) k_recolour_tri_lights(rayhip_light *__restrict__ lights, const uint32_t n_lights, const uint16_t *__restrict__ light_emitter,
                                                            const uint32_t *__restrict__ claim, const rayhip_material *__restrict__ materials,
                                                            const uint32_t n_materials) {
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li < n_lights) {
        recolour_tri_light(lights, li, light_emitter, claim, materials, n_materials);
    }
}

} // namespace rayhip_materials
