// hostsim_instances.cpp -- TEST INFRASTRUCTURE.  Moving instances as the device does it (ray_amd/csrc/instances.h: the inverse of a
// transform, the world box of a tree under it, the checks of a call), compiled with g++ (the HOSTSIM_FLAGS of hostsim.cpp: no fma
// contraction, SSE2, glibc libm) over plain arrays, with the prefix hostsim_ and without a context.
// tests/test_instance_pose_hostsim.py holds these against the scenes the reference built and a numpy restatement;
// tests/test_gpu_instance_pose.py holds the device (instances.hip.h) against this file.
//
// Never linked into librayhip.so.
#include <string.h>

#include "../../include/rayhip.h"
#include "../../ray_amd/csrc/instances.h"

#define HS_API extern "C" __attribute__((visibility("default")))

// out[n][16]: the inverses of in[n][16]
HS_API int hostsim_inverse_matrices(const float *in, uint32_t n, float *out) {
    for (uint32_t i = 0; i < n; ++i) {
        rayhip_instances::inverse_matrix(in + size_t(i) * 16, out + size_t(i) * 16);
    }
    return 0;
}

// 1 where all sixteen elements are finite
HS_API int hostsim_finite16(const float *m) { return rayhip_instances::finite16(m) ? 1 : 0; }

// out_boxes[n_slots][6] (lo, hi): the world box of instance slots[k] -- the box of its tree's root node under its transform
HS_API int hostsim_world_boxes(const rayhip_bvh2_node *nodes, uint32_t n_nodes, const rayhip_mesh_instance *instances, uint32_t n_instances,
                               const uint32_t *slots, uint32_t n_slots, float *out_boxes) {
    for (uint32_t k = 0; k < n_slots; ++k) {
        if (slots[k] >= n_instances || instances[slots[k]].node_index >= n_nodes) {
            return 1;
        }
        const rayhip_mesh_instance &mi = instances[slots[k]];
        const rayhip_lbvh::Box b = rayhip_instances::world_box(nodes[mi.node_index], mi.xform);
        memcpy(out_boxes + size_t(k) * 6, &b, sizeof(b));
    }
    return 0;
}

// the whole call over instances[n_instances] in place: flags[n_instances] (1 = the top level names the slot, 2 = a triangle light hangs
// on it), pin_lights = the lights are not refitted.  out_findings[4]: bad slots, duplicates, matrices that are not finite or singular,
// pinned slots.  Returns what the entry point returns (0, 1, 2); the array is written only with 0.
HS_API int hostsim_pose_instances(rayhip_mesh_instance *instances, uint32_t n_instances, const uint8_t *flags, int pin_lights, uint32_t n, const uint32_t *slots,
                                  const float *xforms, uint32_t *out_findings) {
    if (n > 0 && (!slots || !xforms)) {
        return 1;
    }
    return rayhip_instances::pose_instances_host(instances, n_instances, flags, pin_lights != 0, n, slots, xforms, out_findings);
}
